"""-m gpu: the serial path of an active-set trip (csrc/wbc_hex.hpp: hex_gi) -- the nested chain of fast bodies with its one-compare first vote, the
hand-over to the generic loop, the crossbar fetch of the picked row from every source lane.  None of it changes an arithmetic expression, so every
check is the suite's own bar against the oracle plus bit-identity of a robot across batch sizes (one full wavefront, a ragged one, several)."""
import numpy as np
import pytest

import trip_path_states as tps
from test_gpu_parity import TOL_STAND, TOL_TROT, gpu_step, rel_err

pytestmark = pytest.mark.gpu


def _oracle(kind, b, n):
    from oracle import oracle_py as orc
    return orc.step_batch(kind, orc.model(b["model"]), orc.params(kind), b["q"][:, :n], b["v"][:, :n], b["targets"][:, :n], b["mask"][:n])


def _check(kind, cfg, sizes, tol):
    from quadruped_drake_amd import workloads
    b = workloads.make_batch(cfg, n=max(sizes))
    tau_o, met_o, st_o = _oracle(kind, b, max(sizes))
    assert (st_o == 0).all()
    step = lambda n: gpu_step(kind, b["model"], b["q"][:, :n], b["v"][:, :n], b["targets"][:, :n], b["mask"][:n], max_batch=64)
    one = step(1)
    for n in sizes:
        tau, met, st, stats = step(n)
        assert tau.shape == (12, n) and (st == 0).all() and stats["ticks"] == n
        r = rel_err(tau, tau_o[:, :n])
        assert r.max() < tol, (n, r.max())
        assert np.allclose(met, met_o[:, :n], rtol=1e-5, atol=1e-6)
        # robot 0 alone in its wavefront and robot 0 among wave-mates: the same bits
        assert np.array_equal(tau[:, 0], one[0][:, 0]) and np.array_equal(met[:, 0], one[1][:, 0]) and st[0] == one[2][0], n
    return b


def test_fast_path_trot_states():
    """MPTC, config-3 trots: the fast chain alone on most wavefronts.  N = 5: one full wavefront and a ragged one; N = 64: sixteen."""
    _check("mptc", 3, (5, 64), TOL_TROT)


def test_generic_loop_stands():
    """ID, config-2 stands: eight fast bodies, then the generic loop with drops and the W-row fetch."""
    b = _check("id", 2, (8,), TOL_STAND)
    _, _, _, stats = gpu_step("id", b["model"], b["q"], b["v"], b["targets"], b["mask"])
    assert stats["iters_sum"] / stats["ticks"] > 8.0          # (more trips than the fast chain has bodies: the generic loop ran)


@pytest.mark.parametrize("kind", ["mptc", "id"])
def test_every_source_lane_of_the_fetch(kind):
    """Sixteen stands, robot h pushed so that friction row h is the first one added (chosen and checked on the host instantiation:
    tests/test_trip_path_states_cpu.py): the first fetch of the batch reads from source lanes 0 ... 15."""
    from oracle import oracle_py as orc
    q, v, tg, mask = tps.make_states()
    tau, met, st, stats = gpu_step(kind, "mini_cheetah", q, v, tg, mask)
    tau_o, met_o, st_o = orc.step_batch(kind, orc.model("mini_cheetah"), orc.params(kind), q, v, tg, mask)
    assert (st == 0).all() and (st_o == 0).all()
    r = rel_err(tau, tau_o)
    assert r.max() < TOL_STAND, r
    assert np.allclose(met, met_o, rtol=1e-5, atol=1e-6)
    # each robot alone (its row's lane is then the only source of its wavefront's fetch): it runs at least one trip -- it adds a row -- and
    # computes the same bits; the trips of the sixteen add up to the batch's
    trips = 0
    for h in range(16):
        one = gpu_step(kind, "mini_cheetah", q[:, h:h + 1], v[:, h:h + 1], tg[:, h:h + 1], mask[h:h + 1])
        assert one[3]["iters_sum"] >= 1, h
        trips += one[3]["iters_sum"]
        assert np.array_equal(one[0][:, 0], tau[:, h]) and np.array_equal(one[1][:, 0], met[:, h]), h
    assert trips == stats["iters_sum"]
