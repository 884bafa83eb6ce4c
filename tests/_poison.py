"""Poisoned outputs and workspace: a kernel's result must depend on its arguments alone, never on what its output tensors or
the handle's workspace held before the call.  `poisoned` runs one call twice, over two different fills of everything the call
may write or use as scratch, and demands finite, bit-identical results and untouched pad regions."""
import torch

_INT_VIEW = {4: torch.int32, 2: torch.int16}
FILL_A, FILL_B = 0xFF, 0x7F  # f32 / bf16: NaN; 3.39e38 (finite and huge: fmaxf and comparisons drop a NaN, not this)


class IntOut:
    """An integer output (an index map): prefilled with valid in-range values, 0 in round A and `hi` in round B, never a byte
    pattern -- a stale read then gives a wrong answer, not a wild address."""

    def __init__(self, t, hi):
        assert not t.is_floating_point()
        self.t, self.hi = t, int(hi)


def _bits(t):
    return t.view(_INT_VIEW[t.element_size()])


def _word(t, byte):
    v = int.from_bytes(bytes([byte]) * t.element_size(), "little", signed=True)
    return v


def _fill(t, byte):
    assert t.is_floating_point(), "integer outputs go through IntOut"
    _bits(t).fill_(_word(t, byte))


def _holds(t, byte):
    return bool((_bits(t) == _word(t, byte)).all())


def active_handle(dev):
    import vit_amd.functional as vf
    from vit_amd import _cabi

    return vf._HANDLE_OVERRIDE if vf._HANDLE_OVERRIDE is not None else _cabi.handle_for(dev)


def poisoned(dev, run, outs, pads=(), workspace=True):
    """`run()` makes one call (or the fwd + bwd pair of one op) through vit_amd.functional and writes the tensors of `outs`
    (views are fine: the part of a buffer the contract says is written).  `pads`: views of the same buffers the contract says
    are NOT written.  Returns clones of `outs` after round A, in order (IntOut entries as their tensors).
    `workspace=False`: only the outputs are poisoned."""
    h = active_handle(dev)
    run()  # unpoisoned: lets the handle grow the workspace to the call's need (a later regrow would drop the poison)
    ws_ptr = h._ws.data_ptr()
    snaps = []
    for byte in (FILL_A, FILL_B):
        for o in outs:
            if isinstance(o, IntOut):
                o.t.fill_(0 if byte == FILL_A else o.hi)
            else:
                _fill(o, byte)
        for p in pads:
            _fill(p, byte)
        if workspace:
            h.fill_workspace(byte)
        run()
        assert h._ws.data_ptr() == ws_ptr, "the workspace was regrown after it was poisoned"
        for i, p in enumerate(pads):
            assert _holds(p, byte), f"pad region {i} was written (fill {byte:#x})"
        snap = []
        for i, o in enumerate(outs):
            t = o.t if isinstance(o, IntOut) else o
            if t.is_floating_point():
                bad = int((~torch.isfinite(t)).sum())
                assert bad == 0, f"output {i}: {bad} of {t.numel()} elements not finite after fill {byte:#x}"
            snap.append(t.clone())
        snaps.append(snap)
    for i, (a, b) in enumerate(zip(*snaps)):
        if a.is_floating_point():
            a, b = _bits(a), _bits(b)
        diff = int((a != b).sum())
        assert diff == 0, f"output {i}: {diff} of {a.numel()} elements differ between the {FILL_A:#x} and {FILL_B:#x} rounds"
    return snaps[0]
