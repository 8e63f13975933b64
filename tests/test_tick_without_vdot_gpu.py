"""-m gpu: the tick kernels of a handle with NO acceleration buffer bound (wbc_hex_kernel<KIND, TB>: hex_tick<..., VD = false>, csrc/wbc_kernels.hip)
against the kernels that form the accelerations (wbc_hex_kernel<KIND, TB, VdotRows>), which are the only ones a handle launched before the two were split.

launch() picks by `d_vdot != nullptr` (wbc_set_vdot_output), so one handle runs both: a step with no buffer, a step with a buffer bound and a
step after unbinding must give the same torques, metrics and status bit for bit -- the acceleration rows are extra outputs, not another law.
All four laws, torque box off and on, through the C ABI with n = 9 and ld = 12 (two full wavefronts plus one robot: a ragged last workgroup,
and padding columns that every output has to leave alone), on a batch of trot states (the fast path of the active set) and on a batch of
4-contact stands (the generic loop, where rows get dropped).  The bound buffer is checked against x[:18] of the oracle's literal QP at the bar
of tests/test_rollout.py (1e-8, relative to 1 + max|x|), and kernel_info() -- which reports the kernel the handle would launch NOW -- must show
no scratch in either state."""
import ctypes as C

import numpy as np
import pytest

import plant_edges as pe
from poisons import POISONS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["id", "mptc", "pc", "clf"]
BOX = {"id": 12.0, "clf": 12.0, "mptc": 10.0, "pc": 10.0}     # N m, as tests/test_robustness_gpu.py: binds on part of a batch
N, LD = 9, 12


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _ptr(x):
    return C.c_void_p(x.data_ptr())


def _preset(rows, dtype=np.float64):
    return _t(np.full((rows, LD) if rows else (LD,), pe.sentinel(dtype), dtype))


def _cls(kind):
    from quadruped_drake_amd import IDController, MPTCController, PCController, CLFController
    return {"id": IDController, "mptc": MPTCController, "pc": PCController, "clf": CLFController}[kind]


def _batches():
    from quadruped_drake_amd import workloads
    return {"trot": workloads.make_batch(3, n=N), "stand": workloads.make_batch(2, n=N)}


class _Handle:
    """One controller stepped through the C ABI with ld = 12; every step writes into fresh arrays that hold the sentinels."""

    def __init__(self, kind, box, b):
        from quadruped_drake_amd import _lib
        self.check, self.L = _lib.check, _lib.lib()
        self.ctrl = _cls(kind)(model=b["model"], max_batch=16, device=0, params=({"tau_max": BOX[kind]} if box else None))
        self.inputs = [_t(pe.wide(b[k], LD, fill=np.nan)) for k in ("q", "v", "targets")] + [_t(pe.wide(b["mask"], LD))]

    def bind(self, vd):
        self.check(self.L.wbc_set_vdot_output(self.ctrl._h, None if vd is None else _ptr(vd)))

    def step(self):
        tau, met, st = _preset(12), _preset(4), _preset(0, np.int32)
        self.ctrl._bind_stream()
        q, v, tg, mk = self.inputs
        self.check(self.L.wbc_step(self.ctrl._h, N, LD, _ptr(q), _ptr(v), _ptr(tg), _ptr(mk), None, None, _ptr(tau), _ptr(met), _ptr(st)))
        self.ctrl.sync()
        return dict(tau=tau.cpu().numpy(), met=met.cpu().numpy(), st=st.cpu().numpy())

    def close(self):
        self.ctrl.close()


@pytest.mark.parametrize("box", [False, True], ids=["nobox", "box"])
@pytest.mark.parametrize("kind", KINDS)
def test_unbound_bound_and_unbound_again_give_the_same_bits(kind, box):
    from oracle import oracle_py as orc
    compared = 0
    for name, b in _batches().items():
        h = _Handle(kind, box, b)
        info_unbound = h.ctrl.kernel_info()
        first = h.step()
        vd = _preset(18)
        h.bind(vd)
        info_bound = h.ctrl.kernel_info()
        bound = h.step()
        vd_bound = vd.cpu().numpy()
        h.bind(None)
        info_after = h.ctrl.kernel_info()
        vd.copy_(_preset(18))                    # the SAME buffer, re-filled in place: the step after unbinding must not touch it
        again = h.step()
        vd_after = vd.cpu().numpy()
        h.close()
        assert info_after == info_unbound, (name, info_after, info_unbound)
        print("VDOT-SWITCH %s box %d %s: status %s, kernel_info unbound %s bound %s" % (kind, box, name, first["st"][:N].tolist(), info_unbound, info_bound))
        assert info_unbound["scratch_bytes_per_lane"] == 0 and info_bound["scratch_bytes_per_lane"] == 0
        for k in ("tau", "met", "st"):
            assert pe.padding_kept(first[k], N) and pe.padding_kept(bound[k], N) and pe.padding_kept(again[k], N), (name, k)
            assert pe.same_bits(first[k], bound[k]), (name, k)
            assert pe.same_bits(first[k], again[k]), (name, k)
            assert not (pe.bits(first[k][..., :N]) == pe.bits(np.array(pe.sentinel(first[k].dtype)))).any(), (name, k)   # every entry was written
        assert np.isfinite(first["tau"][:, :N]).all() and np.isfinite(first["met"][:, :N]).all()
        # the bound buffer: rows 0..17 of the n columns written (finite, no sentinel left), the padding columns as they were
        assert np.isfinite(vd_bound[:, :N]).all() and not (pe.bits(vd_bound[:, :N]) == pe.bits(np.array(pe.SENT_F64))).any(), name
        assert pe.padding_kept(vd_bound, N), name
        assert pe.padding_kept(vd_after, 0), name
        # ... and they are the accelerations of the QP (tests/test_rollout.py: test_gpu_vdot_equals_oracle_qp_vd), wherever both sides solved the tick
        m = orc.model(b["model"]); p = orc.params(kind)
        if box:
            p.tau_max = BOX[kind]
        for i in range(N):
            ct = [(int(b["mask"][i]) >> k) & 1 for k in range(4)]
            _, _, st_o, qp = orc.control_law(kind, m, p, b["q"][:, i], b["v"][:, i], b["targets"][:, i], ct, want_qp=True)
            if st_o != 0 or bound["st"][i] != 0:
                continue
            err = np.abs(vd_bound[:, i] - qp["x"][:18]).max()
            assert err < 1e-8 * (1 + np.abs(qp["x"][:18]).max()), (name, i, err)
            compared += 1
    assert compared >= N, compared     # (all of the trot batch at the least when the box is off; part of each batch under a box)


def test_kernel_info_follows_the_binding():
    """The unbound handle runs ANOTHER kernel, and kernel_info() -- which goes through the same tick_kernels() as launch() -- shows it: the register
    total changes when a buffer is bound and comes back when it is unbound.  Two kernels of one law may happen to need the same number of registers
    (the allocator's business), so the difference is asserted where the source says it must exist -- the MPTC tick without a torque box keeps ten
    values fewer alive across the QR and the active set without the rows (profiles/r20/README.md: 438 -> 428); the return to the unbound answer
    is asserted for all eight (law, box) pairs, whose figures are printed."""
    import torch
    b = _batches()["trot"]
    differ = {}
    for kind in KINDS:
        for box in (False, True):
            h = _Handle(kind, box, b)
            unbound = h.ctrl.kernel_info()
            vd = _preset(18)
            h.bind(vd)
            bound = h.ctrl.kernel_info()
            h.bind(None)
            after = h.ctrl.kernel_info()
            h.close()
            assert after == unbound, (kind, box, after, unbound)
            differ[(kind, box)] = (unbound["num_regs"], bound["num_regs"])
    torch.cuda.synchronize()
    print("VDOT-SWITCH registers (unbound, bound): %s" % differ)
    assert differ[("mptc", False)][0] < differ[("mptc", False)][1], differ


@pytest.mark.parametrize("box", [False, True], ids=["nobox", "box"])
@pytest.mark.parametrize("kind", KINDS)
def test_malformed_instance_with_no_buffer_bound(kind, box):
    """Robot 5 -- slot 1 of the second wavefront -- gets a NaN joint angle: status 2 and zero torques as with a buffer bound, finite metrics,
    and not a bit of anybody else moves (the status-2 exit of the tick is one of the places that skip the acceleration rows)."""
    b = _batches()["trot"]
    bad = {k: (np.array(x, copy=True) if isinstance(x, np.ndarray) else x) for k, x in b.items()}
    POISONS["nan_joint"][0](bad, 5)
    h = _Handle(kind, box, b); ref = h.step(); h.close()
    h = _Handle(kind, box, bad); out = h.step(); h.close()
    others = np.arange(N) != 5
    assert out["st"][5] == 2 and (out["tau"][:, 5] == 0).all() and np.isfinite(out["met"][:, 5]).all()
    for k in ("tau", "met", "st"):
        assert pe.padding_kept(out[k], N), k
        assert pe.same_bits(out[k][..., :N][..., others], ref[k][..., :N][..., others]), k
    assert ref["st"][5] != 2
