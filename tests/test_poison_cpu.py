"""The poison table is complete: every exported vit_* name is the entry point of a case of tests/test_poison_gpu.py or is listed
in its EXEMPT dict with a one-line reason, never both.  A new export without either fails here, on the CPU."""
from test_poison_gpu import CASES, EXEMPT

from vit_amd._cabi import _PROTOS


def covered():
    return {e for c in CASES for e in c.entries}


def test_every_export_is_a_case_or_exempt():
    missing = sorted(set(_PROTOS) - covered() - set(EXEMPT))
    assert not missing, f"exports with neither a poison case nor an EXEMPT entry: {missing}"


def test_no_name_is_both_and_none_is_unknown():
    both = sorted(covered() & set(EXEMPT))
    assert not both, f"both a case's entry point and EXEMPT: {both}"
    unknown = sorted((covered() | set(EXEMPT)) - set(_PROTOS))
    assert not unknown, f"not exported: {unknown}"
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in EXEMPT.values())


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
