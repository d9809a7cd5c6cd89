"""The fixtures of tests/test_static_instances_gpu.py can tell the table entries apart: for every net of that test, the
trajectory the fp64 oracles give with ANY other inner activation -- what a wrong entry of the activation ladder would
compute -- lies at least two budgets from the expected one in weights, momentum or outputs (NaN counts as found: the test's
comparisons are false for it).  No GPU: tests/np_oracle.py only."""
import numpy as np
import pytest

from tests import static_instance_cases as fx


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("out_kind", [0, 1], ids=["softmax", "general"])
@pytest.mark.parametrize("dims", fx.SHAPES, ids=["784-300-100-10", "784-100-50-10"])
def test_a_wrong_activation_leaves_the_budgets(oracle_mod, dims, out_kind, bf):
    w_tol, o_tol = fx.budgets(bf)
    for k in range(len(fx.HYPER)):
        w1 = oracle_mod.OracleNet(dims, seed=k + 1).get_weights()           # Random(seed), as the net draws them
        least = float("inf")
        for a in range(5):
            w0 = (w1.astype(np.float32).astype(np.float64) * fx.SCALE[a]).astype(np.float32).astype(np.float64)
            want = fx.trajectory(dims, a, out_kind, bf, k, w0)
            assert all(np.isfinite(x).all() for x in want), "fixture: the oracle has no finite answer (activation %d)" % a
            for b in range(5):
                if b == a:
                    continue
                with np.errstate(all="ignore"):
                    got = fx.trajectory(dims, b, out_kind, bf, k, w0)
                    far = max(np.abs(got[0] - want[0]).max() / w_tol, np.abs(got[1] - want[1]).max() / w_tol, np.abs(got[2] - want[2]).max() / o_tol)
                least = min(least, far) if far == far else least
                assert not far < 2.0, "member %d: activation %d run as %d stays within %.2f budgets" % (k, a, b, far)
        print("wrong-activation distance %s out_kind %d %s member %d: at least %.3g budgets" % ("-".join(map(str, dims)), out_kind, "bf16" if bf else "f32", k, least))
