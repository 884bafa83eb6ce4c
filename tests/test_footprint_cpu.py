"""The footprint table is complete and well formed, and the helper catches what it is for.  Every exported vit_* name is the entry
point of a case of tests/test_footprint_gpu.py or is listed in its NO_FOOTPRINT dict with a one-line reason, never both; every
view a case names exists in what its `make` and `ref` return; every region is large enough for its tolerance; and a `run` that
leaks a neighbouring row fails in each of the three rounds."""
import re

import pytest
import torch

from _footprint import Case, IntIn, footprint, others, rounding_room
from test_footprint_gpu import CASES, NO_FOOTPRINT

from vit_amd._cabi import _PROTOS

CPU = torch.device("cpu")


def covered():
    return {e for c in CASES for e in c.entries}


def test_every_export_is_a_case_or_listed():
    missing = sorted(set(_PROTOS) - covered() - set(NO_FOOTPRINT))
    assert not missing, f"exports with neither a footprint case nor a NO_FOOTPRINT entry: {missing}"


def test_no_name_is_both_and_none_is_unknown():
    both = sorted(covered() & set(NO_FOOTPRINT))
    assert not both, f"both a case's entry point and in NO_FOOTPRINT: {both}"
    unknown = sorted((covered() | set(NO_FOOTPRINT)) - set(_PROTOS))
    assert not unknown, f"not exported: {unknown}"
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in NO_FOOTPRINT.values())


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)


def test_a_case_without_the_nan_round_names_the_line():
    for c in CASES:
        if not c.nan_round:
            assert c.reason and "\n" not in c.reason and re.search(r"[\w/]+\.(hip|h|cpp|py):\d+", c.reason), \
                f"{c.id}: nan_round=False needs a one-line reason with the file:line where the outside value is annihilated"


def test_every_view_exists_and_every_region_has_room():
    """On the host: every case's inputs and reference are built, every target indexes its reference and every outside view its
    input without being empty overall, and the fp64 reference rounded at the kernel's documented rounding points passes each
    region's tolerance with 2 x room (a plain bf16 store has it by construction: 2^-9 < 2e-3)."""
    checked = 0
    for c in CASES:
        d = c.make(CPU)
        refs = c.ref(d) if c.ref is not None else {}
        for name, index in c.views():
            if name in refs:
                assert refs[name][index].numel() > 0, (c.id, name)
                assert name in c.tol, f"{c.id}: no tolerance for {name}"
        for group, regions in zip(c.groups(), c.outside):
            n = 0
            for r in regions:
                name, index = (r.name, r.index) if isinstance(r, IntIn) else r
                assert torch.is_tensor(d[name]), (c.id, name)
                n += d[name][index].numel()
            assert n > 0, f"{c.id}: target {group[0]} declares nothing outside its footprint"
        checked += len(rounding_room(c))
    print(f"{len(CASES)} cases, {sum(len(c.groups()) for c in CASES)} target groups, {checked} regions checked for rounding room")
    assert checked > 0


# ------------------------------------------------------------------ the helper itself, on a pure-torch `run`
def _toy(leak, nan_only=False):
    def make(dev):
        g = torch.Generator().manual_seed(5)
        return {"x": torch.randn(9, 8, generator=g).to(dev), "w": torch.randn(8, generator=g).to(dev)}

    def run(d):
        x = d["x"]
        y = x * d["w"]
        if leak and nan_only:  # reads the next row and multiplies it by zero: only a NaN or an infinity comes through
            y[:-1] = y[:-1] + 0.0 * x[1:]
        elif leak:
            y[:-1] = y[:-1] + leak * x[1:]
        return {"y": y}

    rows = (slice(0, 1), slice(3, 5), slice(8, 9))
    return Case("toy", "toy", make, run, [("y", S) for S in rows], [[("x", others(9, S))] for S in rows],
                ref=lambda d: {"y": d["x"].double() * d["w"].double()}, tol={"y": 4e-3 if leak else 1e-6})


def test_the_helper_passes_a_clean_run():
    footprint(CPU, _toy(0.0), say=lambda *_: None)


@pytest.mark.parametrize("rnd", ["a", "b", "c"])
def test_the_helper_fails_a_leaking_run_in_every_round(rnd):
    """1e-3 x the next row passes the norm-based reference check (the bf16 gate, 4e-3, here) and fails each round on its own."""
    with pytest.raises(AssertionError, match=rf"round \({rnd}\).*outside its footprint"):
        footprint(CPU, _toy(1e-3), rounds=(rnd,), say=lambda *_: None)


def test_a_leak_through_a_zero_weight_shows_in_the_nan_round_alone():
    footprint(CPU, _toy(1.0, nan_only=True), rounds=("a",), say=lambda *_: None)
    with pytest.raises(AssertionError, match=r"round \(c\)"):
        footprint(CPU, _toy(1.0, nan_only=True), rounds=("c",), say=lambda *_: None)


def test_an_integer_region_takes_other_valid_values():
    def make(dev):
        return {"idx": torch.tensor([[0, 2], [1, 3]], dtype=torch.int32), "t": torch.arange(4.0)}

    def run(d):
        assert int(d["idx"].min()) >= 0 and int(d["idx"].max()) < 4
        return {"y": d["t"][d["idx"].long()]}

    footprint(CPU, Case("toy int", "toy", make, run, [("y", 0)], [[IntIn("idx", 1, 0, 4)]]), say=lambda *_: None)
    with pytest.raises(AssertionError, match="outside its footprint"):
        footprint(CPU, Case("toy int wrong", "toy", make, run, [("y", 0)], [[IntIn("idx", 0, 0, 4)]]), say=lambda *_: None)
