"""CPU: the interface of INT8 activations (A20) that needs no device -- the
act_format argument of QuantLinear, the workspace size, and tg_qgemm_act's
argument errors (the convention of test_abi.py::test_argument_errors_without_gpu)."""
import ctypes

import pytest


def test_act_format_argument():
    from gptq_svd_amd.qlinear import INT_ACT_FORMATS, MXQuantLinear, QuantLinear
    assert INT_ACT_FORMATS == {"int8": 2}
    q = QuantLinear(64, 8, 4, 32, act_format="int8")
    assert q.act_format == "int8" and "act_format=int8" in repr(q)
    assert QuantLinear(64, 8, 4, 32).act_format is None
    for bad in ("mxfp8", "int4", 8):
        with pytest.raises(ValueError):
            QuantLinear(64, 8, 4, 32, act_format=bad)
    with pytest.raises(ValueError):
        MXQuantLinear(64, 8, act_format="int8")


P = ctypes.c_void_p(16)
#       T  m   n   group bits act ws
GOOD = (1, 64, 64, 32, 4, 2, P)


@pytest.mark.parametrize("change,index", [({}, 0), (dict(act=1), 14), (dict(bits=5), 13),
                                          (dict(n=48), 11), (dict(n=96, group=48), 12),
                                          (dict(ws=None), 20)])
def test_argument_errors_without_gpu(change, index):
    """Rejected with the argument's index before any device work.  The unchanged
    call passes every check and fails only at the workspace, which is too small."""
    from gptq_svd_amd import _lib as L
    assert L.lib.tg_qgemm_act_workspace_size(1, 64, 64, 32) > 0
    a = dict(zip(("T", "m", "n", "group", "bits", "act", "ws"), GOOD), **change)
    rc = L.lib.tg_qgemm_act(None, P, L.TG_F16, a["T"], a["n"], P, P, P, L.TG_F16, a["m"], a["n"],
                            a["group"], a["bits"], a["act"], None, 0, P, L.TG_F16, a["m"], a["ws"],
                            0)
    assert rc == (-index if index else -99), L.last_error()
    if index:
        assert f"argument {index}".encode() in L.lib.tg_last_error()
