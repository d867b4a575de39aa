"""No device: what gldm_r1d_tile_columns / gldm_r1d_workspace_bytes answer for every row of tests/r1d_envelope_cases.py --
the status of a refused descriptor, the engine geometry and the workspace layout of an accepted one -- and that the table
stands on both sides of every bound of validate() and of the routing predicates of csrc/resnet1d.hip."""
import ctypes

import pytest
import torch

import r1d_envelope_cases as C


def _answers(packed, n):
    from graspldm_amd import _lib
    ptr = ctypes.cast(ctypes.pointer(packed["desc"]), ctypes.c_void_p)
    return _lib.lib().gldm_r1d_tile_columns(ptr), _lib.lib().gldm_r1d_workspace_bytes(ptr, n)


@pytest.mark.parametrize("name", [r.name for r in C.ROWS])
def test_route_and_workspace_of_every_row(name):
    row = C.BY_NAME[name]
    if row.expected == C.PACKER:
        with pytest.raises(ValueError):
            C.pack(name)
        return
    packed = C.pack(name)
    d = packed["desc"]
    assert (d.seq_len, d.emb_dim, d.cond_rows, d.n_levels) == (row.L, row.E, row.cond_rows, len(row.widths))
    assert list(d.dims)[:d.n_levels + 1] == [row.C0, *row.widths]
    if row.expected == C.UNSUPPORTED:
        assert _answers(packed, 7) == (C.UNSUPPORTED, -1)
        return
    for n in (*C.batches(row), 21):
        cols, size = _answers(packed, n)
        assert cols == row.expected.cols, (name, cols)
        assert size == C.workspace_bytes(row, n), (name, n, size)
    assert _answers(packed, 0)[1] == -1


def test_sizes_the_rows_were_written_from():
    """Figures taken from the library when the table was written, against the restated layout."""
    sizes = {("d4_quad_only", 21): 1280, ("d16_quad_only", 7): 1280, ("d16_park_no_chain", 7): 132352,
             ("d16_narrower_then_256", 7): 132352}
    for (name, n), size in sizes.items():
        assert C.workspace_bytes(C.BY_NAME[name], n) == size
        assert _answers(C.pack(name), n)[1] == size


def test_the_table_stands_on_both_sides_of_every_bound():
    """Each bound of validate / pm_supported / pm16_supported / wide_widths / ss_table_rows has a row that meets it and one
    just past it; the rows' own test above pins what the library says for each."""
    acc = {r.name: r for r in C.ROWS if isinstance(r.expected, C.Accept)}
    rej = {r.name: r for r in C.ROWS if not isinstance(r.expected, C.Accept)}

    def some(rows, cond):
        return any(cond(r) for r in rows.values())
    den = lambda r: r.head is None and r.mod is None
    # validate
    assert some(acc, lambda r: r.L == 4) and some(acc, lambda r: r.L == 16) and some(rej, lambda r: r.L == 8)
    assert some(acc, lambda r: len(r.widths) == 6) and some(rej, lambda r: len(r.widths) == 7 and r.expected == C.PACKER)
    assert some(acc, lambda r: len(r.widths) == 1) and some(rej, lambda r: len(r.widths) == 0)
    assert some(acc, lambda r: (r.L, r.E) == (4, 32)) and some(rej, lambda r: (r.L, r.E) == (4, 48))
    assert some(acc, lambda r: (r.L, r.E) == (16, 160)) and some(rej, lambda r: (r.L, r.E) == (16, 176))
    assert some(rej, lambda r: r.E % 16 != 0)
    assert some(acc, lambda r: r.C0 == 4) and some(acc, lambda r: r.C0 == 16) and some(rej, lambda r: r.C0 == 8)
    assert some(acc, lambda r: r.widths[-1] == 256) and some(rej, lambda r: 512 in r.widths)
    assert some(acc, lambda r: 128 in r.widths[:-1]) and some(rej, lambda r: 256 in r.widths[:-1])
    assert some(rej, lambda r: any(w & (w - 1) for w in r.widths))
    assert some(rej, lambda r: r.mod == "groups8")
    # the routing predicates: the 64-column side and the first step off it
    for L, c0, e in ((4, 4, 16), (16, 16, 64)):
        on = lambda r: den(r) and (r.L, r.C0, r.E) == (L, c0, e)
        assert some(acc, lambda r: on(r) and r.expected.cols == 64 and r.cond_rows == 3)
        assert some(acc, lambda r: on(r) and r.expected.cols == 64 and r.cond_rows == 4)   # off the register / LDS fast path
        assert some(acc, lambda r: den(r) and r.L == L and r.C0 != c0 and r.expected.cols == 32)
        assert some(acc, lambda r: den(r) and r.L == L and r.C0 == c0 and r.E != e and r.expected.cols == 32)
        assert some(acc, lambda r: on(r) and 16 in r.widths and r.expected.cols == 32)     # wide_widths
        assert some(acc, lambda r: on(r) and 4 in r.widths and r.expected.cols == 32)
        assert some(acc, lambda r: r.L == L and r.mod == "no_w3" and r.expected.cols == 32)
        for w in (32, 64, 128, 256):
            assert some(acc, lambda r: on(r) and w in r.widths and r.expected.cols == 64)
    assert some(acc, lambda r: r.L == 16 and r.cond_rows == 5 and r.expected.cols == 32)   # pm16_supported
    assert some(acc, lambda r: r.L == 4 and r.cond_rows == 5 and r.expected.cols == 64)    # pm_supported has no such bound
    assert some(acc, lambda r: r.L == 4 and r.head == "decoder" and r.expected.cols == 32)
    # park scratch: the 16-position 64-column engine with a 256-channel last level, with and without the wave-local chain
    assert some(acc, lambda r: r.expected.park and r.widths[:3] == (32, 64, 128))
    assert some(acc, lambda r: r.expected.park and r.widths[:3] != (32, 64, 128))
    assert not some(acc, lambda r: r.expected.park and (r.L != 16 or r.expected.cols != 64 or r.widths[-1] != 256))
    # the per-cloud table: 16 positions, an input layer, E >= 32, dims[0] >= 16 -- on both engines, and each condition missed
    heads = {n: r for n, r in acc.items() if r.head}
    assert some(heads, lambda r: r.expected.table and r.expected.cols == 64)
    assert some(heads, lambda r: r.expected.table and r.expected.cols == 32)
    assert some(heads, lambda r: not r.expected.table and r.L == 4)
    assert some(heads, lambda r: not r.expected.table and r.L == 16 and r.E == 16)
    assert some(heads, lambda r: not r.expected.table and r.L == 16 and r.C0 == 4 and r.E >= 32)
    assert not some(acc, lambda r: r.expected.table and not r.head)
    # encoder heads at the bounds of the latent width
    assert some(acc, lambda r: r.head == ("encoder", 1)) and some(acc, lambda r: r.head == ("encoder", 32))
    assert some(rej, lambda r: r.head == ("encoder", 33) and r.expected == C.PACKER)


@pytest.mark.parametrize("name", C.ACCEPTED)
def test_the_f32_oracle_stays_a_quarter_of_the_bar_from_the_yardstick(name):
    """The f64 yardstick of the GPU tests against the f32 torch oracle on the same inputs (both fed the f32 time-embedding
    rows): within a quarter of the bar, so a GPU failure is the kernel's.  A row that misses this needs another seed."""
    row = C.BY_NAME[name]
    x, z, t = C.inputs(name)
    temb = None
    if row.head is None:
        from graspldm_amd.r1d_pack import time_embedding_table
        temb = time_embedding_table(C.state_dict(name), "", 1000)
    ref = C.forward(name, x, z, t, temb)
    got = C.forward(name, x, z, t, temb, dtype=torch.float32)
    for r, g in zip(ref if row.head else (ref,), got if row.head else (got,)):
        bar = 2e-5 * max(1.0, float(r.abs().max())) if row.head is None else 1e-4
        err = float((g.double() - r).abs().max())
        print(f"{name}: f32 oracle {err:.2e} from f64 (bar {bar:.1e})")
        assert err <= bar / 4, (name, err, bar)
