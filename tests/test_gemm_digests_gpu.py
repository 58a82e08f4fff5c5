"""Every large-M GEMM instance gives the bits it gave before its workgroup prologue, epilogues and launcher moved into
csrc/kernels/gemm_block.h: the digests of tests/gemm_digest_cases.py, recomputed, equal those recorded in
tests/golden/gemm_digests.json on the commit before the move, case by case, refused launches included. Paths A and B
(modes 0 and 1) likewise, against tests/golden/gemv_digests.json, recorded on the commit before path B moved onto that
prologue and every kernel's type switch onto one table. The tolerance is zero; a digest that differs means a
carried-over expression changed."""
import json
import os

import pytest

import gemm_digest_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = {}
for _name in ("gemm_digests.json", "gemv_digests.json"):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", _name)) as _f:
        GOLDEN.update(json.load(_f))


def test_every_recorded_case_belongs_to_an_instance():
    assert {k.split("/")[0] for k in GOLDEN} == set(C.GROUPS) | set(C.GEMV_GROUPS)


@pytest.mark.parametrize("inst", C.instances(), ids=lambda i: i[0])
def test_digests_equal_the_recorded_ones(gpu, inst):
    got = C.run_group(gpu, inst)
    want = {k: v for k, v in GOLDEN.items() if k.split("/")[0] == inst[0]}
    assert set(got) == set(want)
    bad = [k for k in sorted(want) if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} cases differ, e.g. {bad[:8]}"


@pytest.mark.parametrize("inst", C.gemv_instances(), ids=lambda i: i[0])
def test_gemv_digests_equal_the_recorded_ones(gpu, inst):
    got = C.run_gemv_group(gpu, inst)
    want = {k: v for k, v in GOLDEN.items() if k.split("/")[0] == inst[0]}
    assert set(got) == set(want)
    bad = [k for k in sorted(want) if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} cases differ, e.g. {bad[:8]}"
