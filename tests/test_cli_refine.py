"""CLI: --refine_from / --refine_strength parse (CPU) and run end to end on synthetic clouds (GPU), the way
tests/test_cli.py tests the rest."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location("generate_grasps_cli", os.path.join(ROOT, "tools", "generate_grasps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_refine_flags_parse():
    a = _cli().parse_args(["--exp_path", "x", "--mode", "LDM", "--refine_from", "g.npy", "--refine_strength", "0.5"])
    assert a.refine_from == "g.npy" and a.refine_strength == 0.5
    d = _cli().parse_args(["--exp_path", "x"])
    assert d.refine_from is None and d.refine_strength == 0.3


def test_grasp_file_reader(tmp_path):
    cli = _cli()
    H = np.tile(np.eye(4, dtype=np.float32), (5, 1, 1))
    np.save(tmp_path / "a.npy", H)
    np.savez(tmp_path / "b.npz", grasps=np.stack([H, H]))
    assert tuple(cli.read_grasp_file(str(tmp_path / "a.npy")).shape) == (1, 5, 4, 4)
    assert tuple(cli.read_grasp_file(str(tmp_path / "b.npz")).shape) == (2, 5, 4, 4)
    np.savez(tmp_path / "c.npz", poses=H)
    with pytest.raises(SystemExit):
        cli.read_grasp_file(str(tmp_path / "c.npz"))
    np.save(tmp_path / "d.npy", H[:, :3])
    with pytest.raises(SystemExit):
        cli.read_grasp_file(str(tmp_path / "d.npy"))
    with pytest.raises(SystemExit):   # checked before any model is built
        cli.main(["--synthetic", "1024", "--mode", "LDM", "--refine_from", str(tmp_path / "a.npy"), "--refine_strength", "2"])
    with pytest.raises(SystemExit):   # 2 grasp sets for 3 clouds
        cli.main(["--synthetic", "1024", "--mode", "LDM", "--num_samples", "3", "--refine_from", str(tmp_path / "b.npz")])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["LDM", "VAE"])
def test_cli_refine_run(mode, tmp_path):
    """Generate grasps on two synthetic clouds, write them out, hand the file back with --refine_from: --num_grasps comes
    from the file, the result carries the latents, poses are finite proper rotations; with the same seed the clouds are
    the same, and the VAE reconstruction / a strength-0 refinement decode the encoder's mean of exactly those grasps."""
    import torch
    cli = _cli()
    first = str(tmp_path / "first.npz")
    base = ["--synthetic", "1024", "--mode", mode, "--num_samples", "2", "--inference_steps", "10", "--seed", "3"]
    cli.main(base + ["--num_grasps", "5", "--out", first])
    out = str(tmp_path / "second.npz")
    extra = ["--refine_strength", "0.4"] if mode == "LDM" else []
    res = cli.main(base + ["--num_grasps", "9", "--refine_from", first, "--out", out] + extra)
    assert len(res) == 2 and res[0]["grasps"].shape == (1, 5, 4, 4) and res[0]["latent_mu"].shape == (1, 5, 4)
    z = np.load(out)
    H = z["grasps"]
    assert H.shape == (2, 5, 4, 4) and np.isfinite(H).all() and z["latent_mu"].shape == (2, 5, 4)
    R = H[..., :3, :3]
    assert np.allclose(R @ np.swapaxes(R, -1, -2), np.eye(3), atol=1e-4)
    assert ((z["confidence"] > 0) & (z["confidence"] < 1)).all()
    # one [G,4,4] set serves every cloud
    np.save(tmp_path / "one.npy", np.load(first)["grasps"][0])
    res1 = cli.main(base + ["--refine_from", str(tmp_path / "one.npy")] + (["--refine_strength", "0"] if mode == "LDM" else []))
    assert len(res1) == 2 and res1[1]["grasps"].shape == (1, 5, 4, 4) and torch.isfinite(res1[1]["grasps"]).all()
    assert torch.equal(res1[0]["latent_mu"], res[0]["latent_mu"])      # same cloud (seed), same grasps -> same latent
