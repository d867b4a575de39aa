"""One fused encode launch (n grasps) next to one fused decode launch, the twin of run_decode_once.py: the grasp encoder
runs the pose decoder's network, so gldm_decode on the same box and call is its yardstick.  Alternates the two launches,
device events, warmed; prints the mean and the spread over `repeats` blocks of `launches` pairs, and pose_prologue's time.
    python tools/run_encode_once.py [n] [launches] [repeats]"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graspldm_amd import _lib
if os.environ.get("GLDM_LIB"):
    _lib.LIB_PATH = os.environ["GLDM_LIB"]
from graspldm_amd.pipeline import build_fpc_ldm
from graspldm_amd.r1d import pose_prologue
n = int(sys.argv[1]) if len(sys.argv) > 1 else 5120
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 200
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
G = 20 if n % 20 == 0 else 16
dev = torch.device("cuda:0")
ldm = build_fpc_ldm(device=dev)
vae = ldm.vae_model
dec = vae.decoder._get_engine(dev, 3)
enc = vae.encoder.grasp_encoder._get_engine(dev, 3, vae.bottleneck)
z = torch.randn(n // G, 3, 64, device=dev)
zh, h, eps = torch.randn(n, 4, device=dev), torch.randn(n, 7, device=dev), torch.randn(n, 4, device=dev)
H = torch.eye(4, device=dev).repeat(n, 1, 1)
mean, std = torch.zeros(n // G, 6, device=dev), torch.ones(n // G, 6, device=dev)
lab = torch.ones(n, device=dev)
cd, ce = dec.cond_embed(z), enc.cond_embed(z)
runs = dict(decode=lambda: dec.decode(zh, cd, G), encode=lambda: enc.encode(h, ce, G, eps=eps),
            pose_prologue=lambda: pose_prologue(H, lab, mean, std, G))
for f in runs.values():
    for _ in range(20):
        f()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(repeats):
    tot = {k: 0.0 for k in runs}
    evs = []
    for _ in range(launches):
        for k, f in runs.items():   # alternating: decode, encode, prologue, decode, ...
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            evs.append((k, a, b))
    torch.cuda.synchronize()
    for k, a, b in evs:
        tot[k] += a.elapsed_time(b)
    for k in runs:
        times[k].append(tot[k] / launches)
for k, v in times.items():
    print(f"{k:14s} n={n}: mean {sum(v) / len(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({repeats} x {launches} launches)")
print(f"encode / decode = {sum(times['encode']) / sum(times['decode']):.3f}")
