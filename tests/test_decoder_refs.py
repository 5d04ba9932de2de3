"""The checkers of tests/decoder_ref.py have teeth (CPU): a plain f32 restatement of k_attn_ragged's algorithm satisfies the
assertion of every attention case of tests/test_gpu_decoder_edges.py, and each of six single defects of that algorithm -- a
causal mask off by one either way, a dropped key, two exchanged V rows, a missing accumulator rescale, an unscaled merge of the
four streams -- fails at least one case.  That is what makes a pass of the GPU test say something about the kernel."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import decoder_ref as R  # noqa: E402

CASES = R.attn_cases()


def _run(c, defect=None):
    case = R.build_attn_case(c)
    out = R.attn_emulated(case["q"], case["k"], case["v"], case["pos"], case["row_of"], defect=defect)
    return R.attn_violations(out, case)


def test_case_table():
    assert len(CASES) == 20 and len({R.case_id(c) for c in CASES}) == 20
    assert {c.kind for c in CASES} == set(R.KINDS) and sum(1 for c in CASES if c.rows) == len(R.KINDS)
    for c in CASES:
        rep_rows = c.H // c.KVH * c.T
        assert c.t_max == 4096 and rep_rows in (20, 63)
        case = R.build_attn_case(c)
        n_tiles = int(case["pos"].max()) // 32 + 1
        assert c.pos0[0] == 0 or (n_tiles % 4 != 0 and (int(case["pos"].max()) + 1) % 32 != 0)   # ragged last tile
    seen = set()
    for c in CASES:
        if c.kind == "needle":
            case = R.build_attn_case(c)
            seen |= {i for i, n in enumerate(case["count"]) if n > 0}
    assert seen == set(range(len(R.NEEDLES)))                     # every needle is chosen by a row of some case


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_clean_emulation_satisfies_every_case(c):
    bad, worst = _run(c)
    print(f"{R.case_id(c)}: worst |err| / bound {worst:.3f}")
    assert bad == 0, (bad, worst)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_fails_a_case(defect):
    caught = []
    for c in CASES:
        bad, worst = _run(c, defect)
        if bad:
            caught.append((R.case_id(c), bad, round(worst, 2)))
    print(f"{defect}: caught by {len(caught)} of {len(CASES)} cases: {caught}")
    assert caught
