"""Every large-M GEMM instance gives the bits it gave before its workgroup prologue, epilogues and launcher moved into
csrc/kernels/gemm_block.h: the digests of tests/gemm_digest_cases.py, recomputed, equal those recorded in
tests/golden/gemm_digests.json on the commit before the move, case by case, refused launches included. The tolerance
is zero; a digest that differs means a carried-over expression changed."""
import json
import os

import pytest

import gemm_digest_cases as C

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_digests.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_recorded_case_belongs_to_an_instance():
    assert {k.split("/")[0] for k in GOLDEN} == set(C.GROUPS)


@pytest.mark.parametrize("inst", C.instances(), ids=lambda i: i[0])
def test_digests_equal_the_recorded_ones(gpu, inst):
    got = C.run_group(gpu, inst)
    want = {k: v for k, v in GOLDEN.items() if k.split("/")[0] == inst[0]}
    assert set(got) == set(want)
    bad = [k for k in sorted(want) if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} cases differ, e.g. {bad[:8]}"
