"""The planner's output, byte for byte: for every case of tests/plan_digest.py the plan built by libtssplat_amd.so
(``host_only=True``: no HIP) hashes to the digest recorded in tests/golden/plan_digests.json -- plan_info(), every tile's
descriptor fields, planes, row table, vertex ids, destinations, slot tets and rest positions, the finish lists, the adjacency
and index_reps().  The golden file is recorded before a change of the planner (tests/golden/make_golden.py plan_digests),
never after it."""
import json

import pytest

import plan_digest as PD


@pytest.fixture(scope="module")
def golden():
    with open(PD.GOLDEN) as fh:
        return json.load(fh)


def test_golden_file_lists_exactly_the_cases(golden):
    assert sorted(golden) == sorted(PD.case_id(*c) for c in PD.CASES)


@pytest.mark.parametrize("case", PD.CASES, ids=[PD.case_id(*c) for c in PD.CASES])
def test_plan_bytes_are_the_recorded_ones(golden, case):
    want = golden[PD.case_id(*case)]
    kind, spheres, kw, operator = case
    from tssplat_amd import tet_spheres_ext as ext
    rest, tets, L = PD.make_inputs(kind, spheres, operator)
    assert PD.input_digest(rest, tets, L) == want["inputs"], \
        "the INPUTS differ from the recorded ones (scene generator / numpy of this environment), not the planner"
    ts = ext.TetSpheres(rest.reshape(-1), tets.reshape(-1), host_only=True, operator=L, **kw)
    assert PD.plan_digest(ts) == want["plan"], "the planner built other bytes than the recorded plan"
