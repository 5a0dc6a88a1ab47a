"""tests/arena.py finds what it claims to find: three fake "entries" written in torch (CPU tensors), each with one
planted defect, must be reported with the right kind and place, and a clean one must pass."""
import numpy as np
import torch

import arena
from arena import Arena, run_independent

DEV = torch.device("cpu")
WS = 64   # bytes the fake entries ask for


def _x():
    return {"x": torch.arange(1.0, 9.0, dtype=torch.float64)}


def _beyond(v, k):
    """Element ``k`` of ``v``'s storage counted from v's start (k < 0 or k >= numel: outside the view)."""
    return v.as_strided((1,), (1,), v.storage_offset() + k)


def clean(inp, ws, out):
    buf = ws.get(WS, DEV)
    buf[:WS].fill_(0x5A)   # scratch written before it is read
    return {"y": inp["x"] * 2 + buf[:8].view(torch.float64) * 0}


def reads_workspace(inp, ws, out):
    buf = ws.get(WS, DEV)
    return {"y": inp["x"] * 2 + buf[:8].view(torch.float64)}


def writes_past_workspace(inp, ws, out):
    buf = ws.get(WS, DEV)
    _beyond(buf, WS).fill_(0x5A)
    return {"y": inp["x"] * 2}


def reads_before_input(inp, ws, out):
    x = inp["x"]
    return {"y": x * 2 + _beyond(x, -1)}


def test_arena_views_are_aligned_guarded_and_disjoint():
    ar = Arena(DEV, 1 << 16)
    a = ar.take((3, 5), torch.complex128, name="a")
    ws = [ar.workspace(100, offset=o, name=f"ws{o}") for o in (0, 8, 16, 248)]
    assert a.shape == (3, 5) and a.dtype == torch.complex128 and a.is_contiguous() and a.data_ptr() % 512 == 0
    for w, o in zip(ws, (0, 8, 16, 248)):
        assert w.buf.numel() == 100 and w.buf.dtype == torch.uint8 and w.buf.data_ptr() % 512 == o
    assert len(ar.bands) == 10
    p0 = ar.buf.data_ptr()
    for name, v in ar.views.items():
        lo, hi = v.data_ptr() - p0, v.data_ptr() - p0 + v.numel() * v.element_size()
        before, after = [b for b in ar.bands if b.owner == name]
        assert (before.side, after.side) == ("before", "after")
        assert before.hi == lo and before.hi - before.lo >= arena.GUARD and after.lo == hi and after.hi - hi == arena.GUARD
    spans = sorted((b.lo, b.hi) for b in ar.bands)
    assert all(s[1] <= t[0] for s, t in zip(spans, spans[1:]))   # bands never overlap (nor cover a view)
    assert ws[0].get(100, DEV) is ws[0].buf and ws[0].get(64, DEV) is ws[0].buf   # what every wrapper's workspace= does


def test_fill_and_guards_intact_report_offsets():
    ar = Arena(DEV, 1 << 15)
    v = ar.take((16,), torch.float64, name="v")
    for byte in arena.FILLS:
        ar.fill(ar.bands, byte)
        ar.fill(v, 0x11)
        assert ar.guards_intact(byte) == []
        assert bool((v.view(torch.uint8) == 0x11).all())
    lo = v.data_ptr() - ar.buf.data_ptr()
    ar.buf[lo + 128 + 3] = 7          # the 4th byte after the view
    ar.buf[lo - 2] = 7                # the 2nd byte before it
    hits = {h.side: h for h in ar.guards_intact(0xFF)}
    assert (hits["after"].owner, hits["after"].distance, hits["after"].offset, hits["after"].count) == ("v", 3, lo + 131, 1)
    assert (hits["before"].owner, hits["before"].distance, hits["before"].offset) == ("v", 2, lo - 2)


def test_clean_entry_passes_every_step():
    rep = run_independent(clean, label="clean", device=DEV, inputs=_x(), predecessor=lambda ws: ws.get(32, DEV).fill_(3),
                          offsets=arena.OFFSETS)
    print(rep.line())
    assert rep.ok, rep
    assert rep.ws_bytes == WS and rep.steps == ["control", "fill", "history", "alignment", "bounds"]


def test_history_step_with_a_larger_predecessor():
    seen = []

    def pred(ws):
        seen.append(ws.get(4 * WS, DEV).numel())
        ws.buf.fill_(0x40)   # (doubles of 32.5...)

    rep = run_independent(clean, label="clean", device=DEV, inputs=_x(), predecessor=pred)
    assert rep.ok and seen == [4 * WS, 4 * WS], (rep, seen)   # (the sizing call, then the arena's view of that size)
    rep = run_independent(reads_workspace, label="reads-ws", device=DEV, inputs=_x(), fills=(0x00,), predecessor=pred)
    assert rep.kinds() == {"history-dependent"}, rep


def test_workspace_read_is_reported_as_workspace_dependent():
    rep = run_independent(reads_workspace, label="reads-ws", device=DEV, inputs=_x())
    print(rep.line())
    assert "workspace-dependent" in rep.kinds() and "guard-dependent" not in rep.kinds(), rep
    assert "nan" in rep.kinds() and "out-of-bounds" not in rep.kinds(), rep   # (0xFF doubles are NaN)
    assert [f.step for f in rep.findings if f.kind == "workspace-dependent"] == ["fill 0xFF"]


def test_write_past_the_workspace_is_reported_with_its_offset():
    rep = run_independent(writes_past_workspace, label="writes-past", device=DEV, inputs=_x(), workspace=WS)
    print(rep.line())
    assert rep.kinds() == {"out-of-bounds"}, rep
    for f in rep.findings:   # every run writes it: the control's two and the 0xFF one
        (h,) = f.hits
        assert (h.owner, h.side, h.distance, h.count) == ("ws", "after", 0, 1), f
    assert {f.step for f in rep.findings} == {"control", "fill 0xFF"}


def test_read_before_an_input_is_reported_as_guard_dependent():
    rep = run_independent(reads_before_input, label="reads-before", device=DEV, inputs=_x(), workspace=False)
    print(rep.line())
    assert "guard-dependent" in rep.kinds() and "workspace-dependent" not in rep.kinds(), rep
    assert "out-of-bounds" not in rep.kinds(), rep
    # and with a workspace in play the dependence is still put on the guards
    def both(inp, ws, out):
        ws.get(WS, DEV)
        return reads_before_input(inp, ws, out)
    rep = run_independent(both, label="reads-before", device=DEV, inputs=_x(), workspace=WS)
    assert "guard-dependent" in rep.kinds() and "workspace-dependent" not in rep.kinds(), rep


def test_nondeterministic_entry_fails_its_control():
    n = [0]

    def drifting(inp, ws, out):
        n[0] += 1
        return {"y": inp["x"] + n[0]}

    rep = run_independent(drifting, label="drifting", device=DEV, inputs=_x(), workspace=False)
    assert rep.kinds() == {"nondeterministic"} and rep.steps == ["control"], rep


def test_out_buffers_are_arena_views_with_guards():
    def entry(inp, ws, out):
        out["y"].copy_(inp["x"] * 2)
        _beyond(out["y"].view(torch.uint8), 64).fill_(0x5A)   # one byte past the output
        return {"y": out["y"]}

    rep = run_independent(entry, label="out", device=DEV, inputs=_x(), outs={"y": ((8,), torch.float64)}, workspace=False)
    assert rep.kinds() == {"out-of-bounds"}, rep
    h = rep.findings[0].hits[0]
    assert (h.owner, h.side, h.distance, h.count) == ("y", "after", 0, 1)


def test_raw_bytes_tells_signed_zeros_and_nan_payloads_apart():
    a, b = np.array([0.0, np.nan]), np.array([-0.0, np.nan])
    assert not np.array_equal(arena.raw_bytes(a), arena.raw_bytes(b))
    assert np.array_equal(arena.raw_bytes(torch.from_numpy(a)), arena.raw_bytes(a))
