"""An arena of guarded device views, and the driver that checks an entry against the memory it is given.

Every asynchronous ``*_batch`` entry works inside a workspace its caller owns; in production that is the package-wide
``solver._DEFAULT_WS``, which always holds what the previous entry left there at another shape and layout.  The
helpers here hand an entry its workspace, its inputs and (where the wrapper takes ``out=``) its outputs as views of
one ``torch.uint8`` buffer, each between two guard bands, and then vary what the entry must not depend on:

  control     the same arena and fill twice: the outputs must be bit-identical (run-to-run determinism)
  fill        workspace and guard bands filled with 0x00, then with 0xFF (NaN doubles, -1 ints: the library's own
              ACE_POISON pattern): the outputs must not change and must hold no NaN
  history     another entry (or shape) runs through the same workspace first, nothing is refilled
  bounds      after every run each guard band still equals its fill
  alignment   the 0xFF run again with the workspace view 8, 16 and 248 bytes past a 512-byte boundary

Every comparison is on the raw bytes of the outputs (no tolerance).  This is a plain module: no fixtures, no pytest
settings.  It runs on CPU tensors too (tests/test_arena.py plants the defects it claims to find).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

ALIGN = 512
GUARD = 4096
FILLS = (0x00, 0xFF)
OFFSETS = (8, 16, 248)


@dataclass
class Band:
    """One guard band: arena bytes [lo, hi) before or after the view called ``owner``."""
    lo: int
    hi: int
    owner: str
    side: str   # "before" | "after"


@dataclass
class Hit:
    """A changed guard byte.  ``distance``: bytes past the view's end (side "after": 0 is the first byte after it), or
    bytes before its start (side "before": 1 is the byte just before it)."""
    offset: int   # in the arena
    owner: str
    side: str
    distance: int
    count: int    # changed bytes in this band


class Arena:
    """One uint8 buffer handing out contiguous views, each with a guard band on both sides."""

    def __init__(self, device, nbytes):
        self.device = torch.device(device)
        self.raw = torch.zeros(int(nbytes) + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.raw.data_ptr()) % ALIGN   # arena offset 0 sits on a 512-byte boundary
        self.buf = self.raw[self.base:self.base + int(nbytes)]
        self.top = 0
        self.bands: list[Band] = []
        self.views: dict[str, torch.Tensor] = {}

    @staticmethod
    def room(nbytes, guard=GUARD):
        """Arena bytes one view of ``nbytes`` takes at most (guards, alignment and an offset below 512 included)."""
        return int(nbytes) + 2 * guard + 2 * ALIGN

    def take(self, shape, dtype, align=ALIGN, guard=GUARD, offset=0, name=None):
        """A contiguous view of ``shape`` / ``dtype`` that starts ``offset`` bytes past an ``align`` boundary."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = item * int(np.prod(shape, dtype=np.int64))
        start = -(-(self.top + guard) // align) * align + offset
        end = start + nbytes
        if end + guard > self.buf.numel():
            raise ValueError(f"arena of {self.buf.numel()} B is too small for a view of {nbytes} B at {start}")
        name = name or f"view{len(self.views)}"
        self.bands.append(Band(self.top, start, name, "before"))
        self.bands.append(Band(end, end + guard, name, "after"))
        self.top = end + guard
        v = self.buf[start:end].view(dtype).reshape(shape)
        assert v.data_ptr() % align == offset % align and v.is_contiguous()
        self.views[name] = v
        return v

    def put(self, src, name=None, **kw):
        """An arena view holding a copy of ``src``."""
        v = self.take(src.shape, src.dtype, name=name, **kw)
        v.copy_(src)
        return v

    def workspace(self, nbytes, offset=0, name="ws"):
        """A ``solver.Workspace`` whose ``.buf`` is an arena view of exactly ``nbytes`` bytes, ``offset`` bytes past a
        512-byte boundary (``Workspace.get`` returns ``.buf`` unchanged when it is large enough)."""
        from ace_amd.solver import Workspace
        ws = Workspace()
        ws.buf = self.take((nbytes,), torch.uint8, offset=offset, name=name)
        return ws

    def fill(self, what, byte):
        """Fill a view, or a list of guard bands (``arena.bands``), with ``byte``."""
        if isinstance(what, torch.Tensor):
            what.view(torch.uint8).fill_(byte)
            return
        for b in what:
            self.buf[b.lo:b.hi].fill_(byte)

    def guards_intact(self, byte):
        """Compare every guard band with ``byte`` (on the device): the changed bytes, [] if every band is intact."""
        bad = [(self.buf[b.lo:b.hi] != byte) for b in self.bands]
        flags = torch.stack([m.any() for m in bad]).cpu().numpy() if bad else []
        hits = []
        for b, m, f in zip(self.bands, bad, flags):
            if f:
                pos = m.nonzero().reshape(-1).cpu().numpy() + b.lo
                first = int(pos[0] if b.side == "after" else pos[-1])
                dist = first - b.lo if b.side == "after" else b.hi - first
                hits.append(Hit(first, b.owner, b.side, dist, len(pos)))
        return hits


@dataclass
class Finding:
    kind: str     # nondeterministic | workspace-dependent | guard-dependent | fill-dependent | history-dependent |
                  # alignment-dependent | out-of-bounds | nan | workspace-replaced
    step: str
    detail: str
    hits: list = field(default_factory=list)

    def __str__(self):
        return f"[{self.step}] {self.kind}: {self.detail}"


@dataclass
class Report:
    label: str
    ws_bytes: int
    steps: list = field(default_factory=list)
    findings: list = field(default_factory=list)

    @property
    def ok(self):
        return not self.findings

    def kinds(self):
        return {f.kind for f in self.findings}

    def line(self):
        return f"arena {self.label}: workspace {self.ws_bytes} B, steps {'+'.join(self.steps)}, " + (
            "ok" if self.ok else "; ".join(str(f) for f in self.findings))

    def __str__(self):
        return self.line()


def raw_bytes(t):
    """The raw bytes of a tensor (or array) as a host uint8 array."""
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous().cpu().numpy()
    return np.ascontiguousarray(t).reshape(-1).view(np.uint8)


def _has_nan(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return t.dtype.kind in "fc" and bool(np.isnan(t).any())


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def run_independent(call, fills=FILLS, *, label, device, inputs, outs=None, workspace=True, predecessor=None,
                    offsets=(), nan_ok=(), guard=GUARD):
    """Run ``call`` under the protocol of the module docstring and report what it depends on.

    call(inp, ws, out) -> {name: tensor}: one run of the entry.  ``inp``: {name: tensor} of its inputs, ``ws``: the
        ``solver.Workspace`` to pass as ``workspace=`` (None for an entry without one), ``out``: {name: tensor} of
        the buffers for ``out=`` (empty where the wrapper has none).  The returned outputs are compared.
    inputs: {name: tensor}; each is copied into an arena view at 512-byte alignment.
    outs: {name: (shape, dtype)} of arena views for ``out=``.
    workspace: True: the entry's request is learnt from a first call with a plain ``Workspace()`` (afterwards its
        ``.buf.numel()``); an int: that many bytes; False: the entry has no workspace (control and bounds only).
    predecessor(ws): runs another entry or shape through ``ws`` (the history step); None: no history step.
    offsets: workspace offsets past a 512-byte boundary for the alignment step.
    nan_ok: names of outputs that hold NaN by definition.
    """
    outs = outs or {}
    dev = torch.device(device)
    ws_bytes = 0
    if workspace is True:
        from ace_amd.solver import Workspace
        probe = Workspace()
        call(dict(inputs), probe, {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in outs.items()})
        _sync(dev)
        ws_bytes = int(probe.buf.numel())
    elif workspace:
        ws_bytes = int(workspace)
    pred_bytes = 0
    if predecessor is not None and ws_bytes:
        from ace_amd.solver import Workspace
        probe = Workspace()
        predecessor(probe)
        _sync(dev)
        pred_bytes = int(probe.buf.numel())
    item = lambda d: torch.empty((), dtype=d).element_size()   # noqa: E731
    total = sum(Arena.room(t.numel() * t.element_size(), guard) for t in inputs.values())
    total += sum(Arena.room(int(np.prod(s, dtype=np.int64)) * item(d), guard) for s, d in outs.values())
    total += (1 + len(offsets)) * Arena.room(ws_bytes, guard) if ws_bytes else 0
    total += Arena.room(pred_bytes, guard) if pred_bytes > ws_bytes else 0
    ar = Arena(dev, total)
    inp = {k: ar.put(t, name=k, guard=guard) for k, t in inputs.items()}
    out = {k: ar.take(s, d, name=k, guard=guard) for k, (s, d) in outs.items()}
    ws = ar.workspace(ws_bytes, name="ws") if ws_bytes else None
    shifted = [ar.workspace(ws_bytes, offset=o, name=f"ws+{o}") for o in offsets] if ws_bytes else []
    hist = ar.take((pred_bytes,), torch.uint8, name="ws-history", guard=guard) if pred_bytes > ws_bytes else None
    rep = Report(label, ws_bytes)

    def ar_ws(view):
        from ace_amd.solver import Workspace
        w = Workspace()
        w.buf = view
        return w

    def run(w, step):
        view = None if w is None else w.buf
        res = call(inp, w, out)
        _sync(dev)
        if w is not None and w.buf is not view:
            rep.findings.append(Finding("workspace-replaced", step, "the wrapper did not take the arena's workspace"))
        return {k: (raw_bytes(v), _has_nan(v)) for k, v in res.items()}

    def fill(w, ws_byte, guard_byte):
        for v in ([w.buf] if w is not None else []) + list(out.values()):
            ar.fill(v, ws_byte)
        ar.fill(ar.bands, guard_byte)

    def differ(a, b):
        return [k for k in a if a[k][0].shape != b[k][0].shape or not np.array_equal(a[k][0], b[k][0])]

    def bounds(step, byte):
        hits = ar.guards_intact(byte)
        if hits:
            rep.findings.append(Finding("out-of-bounds", step, "; ".join(
                f"{h.count} byte(s) changed {h.side} {h.owner}, nearest at distance {h.distance} (arena offset "
                f"{h.offset})" for h in hits), hits))

    # ---- control: twice with the same arena and the same fill
    f0 = fills[0]
    fill(ws, f0, f0)
    ref = run(ws, "control")
    bounds("control", f0)
    fill(ws, f0, f0)
    again = run(ws, "control")
    bounds("control", f0)
    rep.steps.append("control")
    d = differ(ref, again)
    if d:
        rep.findings.append(Finding("nondeterministic", "control", f"outputs {d} differ between two identical runs"))
        return rep
    nans = [k for k in ref if ref[k][1] and k not in nan_ok]
    if nans:
        rep.findings.append(Finding("nan", "control", f"outputs {nans} hold NaN"))

    # ---- fill independence (and which memory a dependence is on)
    for f in fills[1:]:
        step = f"fill 0x{f:02X}"
        fill(ws, f, f)
        got = run(ws, step)
        bounds(step, f)
        d = differ(ref, got)
        if d:
            kinds = []
            if ws is not None:
                fill(ws, f, f0)
                if differ(ref, run(ws, step)):
                    kinds.append("workspace-dependent")
            fill(ws, f0, f)
            if differ(ref, run(ws, step)):
                kinds.append("guard-dependent")
            for kind in kinds or ["fill-dependent"]:
                rep.findings.append(Finding(kind, step, f"outputs {d} change with the fill"))
        nans = [k for k in got if got[k][1] and k not in nan_ok]
        if nans:
            rep.findings.append(Finding("nan", step, f"outputs {nans} hold NaN"))
    if len(fills) > 1:
        rep.steps.append("fill")
    last = fills[-1]

    # ---- history independence: another entry through the same workspace first, nothing refilled
    if predecessor is not None and ws is not None:
        if hist is None:     # the predecessor fits: the very workspace the 0xFF run just left
            hw, pw = ws, ar_ws(ws.buf)
        else:                # it asks for more: both start at one base, the case leaves its data there first
            hw, pw = ar_ws(hist[:ws_bytes]), ar_ws(hist)
            ar.fill(hist, last)
            run(hw, "history")
        pview = pw.buf
        predecessor(pw)
        _sync(dev)
        if pw.buf is not pview:
            rep.findings.append(Finding("workspace-replaced", "history", "the predecessor left the arena's workspace"))
        got = run(hw, "history")
        bounds("history", last)
        d = differ(ref, got)
        if d:
            rep.findings.append(Finding("history-dependent", "history", f"outputs {d} change after a predecessor"))
        rep.steps.append("history")

    # ---- workspace alignment
    for w, o in zip(shifted, offsets):
        step = f"alignment +{o}"
        fill(w, last, last)
        got = run(w, step)
        bounds(step, last)
        d = differ(ref, got)
        if d:
            rep.findings.append(Finding("alignment-dependent", step, f"outputs {d} change with the workspace offset"))
    if shifted:
        rep.steps.append("alignment")
    rep.steps.append("bounds")
    return rep
