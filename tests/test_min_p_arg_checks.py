"""Which status code the three min-p entry points return for a bad min_p, and that min_p <= 0 is the top-k entry point's call:
the same code for the same (rejected or empty) call.  Every call here returns before any launch, so no GPU is needed -- and
none is allowed: the pointers are made-up addresses (tests/test_sampling_arg_checks.py)."""
import pytest

from tests.test_sampling_arg_checks import (A, ALIGNMENT, BAD_DTYPE, DRAFT, INVALID, NAN, ODD_V, OK, RESIDUAL, UNSUPPORTED, V,
                                            VERIFY, WORKSPACE, _D, _R, _V, _VO, _W)

ENTRY = {
    "asd_draft_sample_min_p": (DRAFT, _D + ["top_k", "top_p", "min_p", "tok", "lp", "thr"] + _W, "asd_draft_sample_top_k"),
    "asd_verify_accept_min_p": (VERIFY, _V + ["top_k", "top_p", "min_p"] + _VO, "asd_verify_accept_top_k"),
    "asd_residual_sample_lp_min_p": (dict(RESIDUAL, lp=A[9]), _R + ["top_k", "top_p", "min_p", "t_threshold", "d_threshold", "token",
                                                                    "lp"] + _W, "asd_residual_sample_lp"),
}
# (what the call changes, the code with a live min_p; None: no expectation of its own, only the off switch is compared)
CHANGES = [
    (dict(), None),                                   # a valid call: never made (it would launch)
    (dict(B=0), OK),
    (dict(B=-1), INVALID),
    (dict(dtype=BAD_DTYPE), UNSUPPORTED),
    (dict(inv_temperature=0.0), INVALID),
    (dict(top_p=NAN), INVALID),
    (dict(V=ODD_V, ld=ODD_V, ld_t=ODD_V, ld_d=ODD_V, ld_b=ODD_V), ALIGNMENT),
]


def _call(lib, name, order, args):
    return getattr(lib, name)(*[args[a] for a in order])


def test_min_p_status_codes_in_the_header_order():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these calls carry made-up device addresses")
    from asd_amd import _binding
    lib = _binding.load_library()
    n = 0
    for name, (defaults, order, sibling) in ENTRY.items():
        sib_order = [a for a in order if a != "min_p"]
        for change, want in CHANGES:
            args = dict(defaults, **{k: v for k, v in change.items() if k in defaults})
            # min_p > 1 or NaN: ASD_ERR_INVALID_ARG ahead of everything, the empty-batch return included
            for bad in (1.5, float("inf"), NAN, 1.0000001):
                assert _call(lib, name, order, dict(args, min_p=bad)) == INVALID, (name, change, bad)
                n += 1
            if not change:
                continue
            # min_p <= 0: the top-k entry point's code for the same arguments
            sib = _call(lib, sibling, sib_order, args)
            for off in (0.0, -0.0, -1.0, float("-inf")):
                assert _call(lib, name, order, dict(args, min_p=off)) == sib, (name, change, off)
                n += 1
            # a live bound: the checks of the top-k entry point with a live top-k
            for live in (1e-30, 0.1, 1.0):
                assert _call(lib, name, order, dict(args, min_p=live)) == want, (name, change, live)
                n += 1
    assert n > 150
    # min-p alone truncates: the verify takes the select's route (alignment is checked), the residual asks for t_threshold and
    # the larger workspace
    d, o, _ = ENTRY["asd_verify_accept_min_p"]
    assert _call(lib, "asd_verify_accept_min_p", o, dict(d, top_p=1.0, min_p=0.1, V=ODD_V, ld=ODD_V)) == ALIGNMENT
    d, o, _ = ENTRY["asd_residual_sample_lp_min_p"]
    plain = lib.asd_residual_sample_workspace_bytes(d["B"], d["V"], d["dtype"])
    assert _call(lib, "asd_residual_sample_lp_min_p", o, dict(d, top_p=1.0, min_p=0.1, t_threshold=None)) == INVALID
    assert _call(lib, "asd_residual_sample_lp_min_p", o, dict(d, top_p=1.0, min_p=0.1, workspace_bytes=plain)) == WORKSPACE
    assert _call(lib, "asd_residual_sample_lp_min_p", o, dict(d, min_p=0.1, lp=None)) == INVALID
