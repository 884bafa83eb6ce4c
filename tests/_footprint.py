"""Input footprints: an output element must depend only on the inputs its header says it depends on.  `footprint` runs one case
once for a baseline, checks every target against an fp64 reference, and then, for each target, runs it three more times with the
input views OUTSIDE that target's footprint overwritten -- (a) by a fresh Gaussian draw of the same scale, (b) by another draw
times 2^12, (c) by the NaN byte fill of tests/_poison.py -- and demands the target bit for bit as in the baseline.  The project
is deterministic (no float atomics, fixed summation orders), so there is no tolerance: a changed bit is a defect, or a sentence
in a header that is not true.  The companion of tests/_poison.py, which pins the same for outputs and workspace."""
import torch

from _poison import FILL_A, _bits, _fill

ROUNDS = ("a", "b", "c")


class IntIn:
    """An integer input region outside a footprint: overwritten by other valid values in [lo, hi), never by a byte pattern -- a
    leak then gives a wrong answer, not a wild address."""

    def __init__(self, name, index, lo, hi):
        self.name, self.index, self.lo, self.hi = name, index, int(lo), int(hi)


class Case:
    """One row of the table.
    make(dev) -> dict of inputs (tensors are cloned before every run, so `run` may work in place; other values pass through)
    run(inputs) -> dict of outputs, one call (or the forward + backward pair of one op) through vit_amd.functional
    targets: [(output name, index)]; outside: for each target, [(input name, index) | IntIn]: what cannot influence it.  A
    target may also be a list of such pairs: views of several outputs that share one footprint and are examined in the same runs.
    A view written (name, index, False) takes part in the bit-equality rounds only: it may be a single row, too small a region
    for the tolerance of the reference check, which larger views of the same output make.
    ref(inputs) -> {output name: fp64 tensor of the whole output}, on the operands as the kernel consumes them; tol: {output
    name: the rel bound its own test file asserts (0: exact)}.  Compared on the target only.
    rounded(inputs) -> as ref, rounded at the kernel's documented rounding points (the CPU check of the 2 x room).
    nan_round=False needs `reason` with the file:line where the kernel reads the outside value and annihilates it.
    every_round(outputs): an assertion made after every run (e.g. rows that must stay exactly zero).
    extra(inputs, outputs): a further assertion on the baseline run (e.g. bit equality with another entry point).
    context(dev): a context manager the runs happen in (options, another handle)."""

    def __init__(self, id, entries, make, run, targets, outside, ref=None, tol=None, rounded=None, nan_round=True, reason=None,
                 every_round=None, context=None, extra=None):
        assert len(targets) == len(outside) and targets, id
        self.id, self.entries = id, (entries,) if isinstance(entries, str) else tuple(entries)
        self.make, self.run, self.targets, self.outside = make, run, list(targets), list(outside)
        self.ref, self.tol, self.rounded = ref, tol or {}, rounded
        self.nan_round, self.reason, self.every_round, self.context, self.extra = nan_round, reason, every_round, context, extra

    def groups(self):
        """The targets as lists of (name, index) pairs, one list per entry of `outside`."""
        return [[v[:2] for v in (t if isinstance(t, list) else [t])] for t in self.targets]

    def views(self):
        """The views the reference check and the rounding-room check look at."""
        return [v[:2] for t in self.targets for v in (t if isinstance(t, list) else [t]) if len(v) == 2 or v[2]]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


def _fresh(inputs):
    return {k: v.clone() if torch.is_tensor(v) else v for k, v in inputs.items()}


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.is_floating_point():
        a, b = _bits(a), _bits(b)
    return int((a != b).sum())


def _perturb(inputs, region, rnd, seed):
    if isinstance(region, IntIn):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        t = inputs[region.name]
        old = t[region.index]
        if old.numel() == 0:
            return 0
        span = region.hi - region.lo
        assert span > 1, "an integer region needs two valid values"
        step = torch.randint(1, span, old.shape, generator=gen).to(old.device)  # never 0: every element changes
        t[region.index] = ((old.long() - region.lo + step) % span + region.lo).to(t.dtype)
        return old.numel()
    name, index = region
    t = inputs[name]
    assert t.is_floating_point(), f"{name}: integer inputs go through IntIn"
    old = t[index]
    if old.numel() == 0:
        return 0
    if rnd == "c":
        new = torch.empty_like(old)
        _fill(new, FILL_A)
    else:
        o = old.double()
        std = float(o.std()) if old.numel() > 1 else 1.0
        gen = torch.Generator(device=old.device).manual_seed(seed)  # drawn where the tensor lives: the regions can be large
        draw = torch.randn(old.shape, generator=gen, dtype=torch.float32, device=old.device).double()
        new = (draw * (std if std > 0 else 1.0) + float(o.mean())) * (4096.0 if rnd == "b" else 1.0)
        new = new.to(t.dtype)
    t[index] = new
    return old.numel()


def check_reference(case, inputs, outputs, say=print):
    """Every target of `outputs` against the fp64 reference at the tolerance of the kernel's own test, on the target alone."""
    if case.ref is None:
        return
    refs = case.ref(inputs)
    for name, index in case.views():
        if name not in refs:
            continue
        got, want, tol = outputs[name][index], refs[name].to(outputs[name].device)[index], case.tol[name]
        if tol == 0:
            assert torch.equal(got.double(), want.double()), f"{case.id}: target {name}{_show(index)} is not the reference exactly"
        else:
            e = rel(got, want)
            say(f"{case.id}: target {name}{_show(index)} rel {e:.3e} (bound {tol:g})")
            assert e < tol, f"{case.id}: target {name}{_show(index)} rel {e:.3e} >= {tol:g}"


def rounding_room(case, dev="cpu"):
    """The CPU check that a region is large enough: the fp64 reference rounded at the kernel's documented rounding points must
    pass the region's tolerance with 2 x room.  Returns [(name, index, rel, tol)] of the targets checked."""
    if case.rounded is None:
        return []
    inputs = case.make(torch.device(dev))
    refs, rounded = case.ref(inputs), case.rounded(inputs)
    seen = []
    for name, index in case.views():
        if name in rounded and case.tol.get(name, 0):
            e = rel(rounded[name][index], refs[name][index])
            seen.append((name, index, e, case.tol[name]))
            assert 2 * e < case.tol[name], f"{case.id}: region {name}{_show(index)} is too small: rounding alone gives {e:.3e}"
    return seen


def _show(index):
    def one(i):
        if isinstance(i, slice):
            return f"{'' if i.start is None else i.start}:{'' if i.stop is None else i.stop}" + (f":{i.step}" if i.step else "")
        if torch.is_tensor(i):
            return f"<{i.numel()} idx>" if i.dtype != torch.bool else f"<mask {int(i.sum())}>"
        return str(i)

    return "[" + ", ".join(one(i) for i in (index if isinstance(index, tuple) else (index,))) + "]"


def footprint(dev, case, rounds=ROUNDS, say=print):
    import contextlib

    dev = torch.device(dev)
    with case.context(dev) if case.context is not None else contextlib.nullcontext():
        pristine = case.make(dev)
        outputs = case.run(_fresh(pristine))
        base = {k: v.clone() for k, v in outputs.items() if torch.is_tensor(v)}
        if case.every_round is not None:
            case.every_round(base)
        check_reference(case, pristine, base, say)
        if case.extra is not None:
            case.extra(pristine, base)
        for ti, (group, regions) in enumerate(zip(case.groups(), case.outside)):
            want = [base[name][index] for name, index in group]
            for (name, index), w in zip(group, want):
                assert w.numel() > 0, f"{case.id}: target {name}{_show(index)} is empty"
                if w.is_floating_point():
                    assert bool(torch.isfinite(w).all()), f"{case.id}: target {name}{_show(index)} is not finite in the baseline"
            for rnd in rounds:
                if rnd == "c" and not case.nan_round:
                    continue
                inputs, moved = _fresh(pristine), 0
                for ri, region in enumerate(regions):
                    moved += _perturb(inputs, region, rnd, 7919 * (ti + 1) + 104729 * ROUNDS.index(rnd) + ri)
                assert moved > 0, f"{case.id}: target {group[0][0]}{_show(group[0][1])} declares nothing outside its footprint"
                got_all = case.run(inputs)
                if case.every_round is not None:
                    case.every_round(got_all)
                for (name, index), w in zip(group, want):
                    diff = _same_bits(got_all[name][index], w)
                    assert diff == 0, (f"{case.id}: round ({rnd}): {diff} of {w.numel()} elements of target {name}{_show(index)} "
                                       f"changed with inputs outside its footprint")
    return base


# ------------------------------------------------------------------ index builders the table shares
def others(n, keep):
    """Index tensor (on the host: it indexes tensors of either device) of the members of range(n) that are not in `keep`, a
    slice, a list or an index tensor."""
    m = torch.ones(n, dtype=torch.bool)
    m[keep] = False
    return m.nonzero().view(-1)
