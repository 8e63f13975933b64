"""The sixteen pushed stands of tests/trip_path_states.py on the HOST instantiation of the kernel header: robot h adds friction row h first (so the batch
reads from every source lane of the active set's crossbar fetch), by a margin no rounding can turn, under both friction-only laws; and the host
instantiation solves them like the oracle (what tests/test_trip_path_gpu.py then asks of the device)."""
import numpy as np
import pytest

import trip_path_states as tps

TOL_STAND = 2e-6     # tests/test_gpu_parity.py: 4-contact stands, ID and MPTC


@pytest.mark.parametrize("kind", ["mptc", "id"])
def test_each_state_adds_its_own_friction_row_first(kind):
    from oracle import oracle_py as orc
    import host_tick as ht
    q, v, tg, mask = tps.make_states()
    rows, margins, adds = tps.first_picks(kind, q, v, tg, mask)
    assert rows == list(range(16)), rows                      # what hex_gi itself added first, recorded by the host instantiation
    assert min(margins) > 1e-2, margins                       # pick keys are coarse at 2^-28: nothing near a tie
    tau, met, st, it = ht.run(kind, orc.load_model_json("mini_cheetah")["flat"], q, v, tg, mask, hexv=True)
    tau_o, met_o, st_o = orc.step_batch(kind, orc.model("mini_cheetah"), orc.params(kind), q, v, tg, mask)
    assert (st == 0).all() and (st_o == 0).all() and (it >= 1).all() and (adds[:, 0] <= it).all()
    rel = np.abs(tau - tau_o).max(0) / np.maximum(np.abs(tau_o).max(0), 1e-3)
    assert rel.max() < TOL_STAND, rel
