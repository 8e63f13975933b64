"""-m gpu: the timing brackets of wbc_time_steps / wbc_time_steps_each (csrc/wbc_kernels.hip: ev0, ev1, evs[]) carry time stamps and nothing
else, so whatever kind of HIP event they are made of (default ones; device-scope and fence-free markers were tried, profiles/r20/README.md),
what must stay true of them needs no tolerance:

  * the device time they report is positive and cannot exceed the host's own clock around the blocking call that queued, ran and read them
    (a marker that fired early or late, or a stamp pair read before the second one landed, breaks one of the two);
  * the launches between them are the launches of K step() calls: the statistics (ticks, iterations, the sixteen contact-mask bins) of
    time_steps(K) equal those of K steps on a fresh handle exactly -- they are read after the stream wait of wbc_stats_get, not through the events.

n = 64 (sixteen wavefronts), K = 4."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, K = 64, 4


def _setup():
    import torch
    from quadruped_drake_amd import MPTCController, workloads
    b = workloads.make_batch(3, n=N)
    ctrl = MPTCController(model=b["model"], max_batch=N, device=0)
    args = [torch.tensor(b[k], device="cuda:0") for k in ("q", "v", "targets", "mask")]
    out = (torch.empty((12, N), dtype=torch.float64, device="cuda:0"), torch.empty((4, N), dtype=torch.float64, device="cuda:0"),
           torch.empty((N,), dtype=torch.int32, device="cuda:0"))
    return ctrl, args, out


def _exact(s):
    return (s["ticks"], s["iters_sum"], s["status_nonzero"], list(s["mask_count"]))


def test_bracketed_time_is_positive_and_inside_the_hosts_clock():
    import torch
    ctrl, args, out = _setup()
    ctrl.step(*args, out=out)                       # (the first launch of a process loads the code object)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ms, _ = ctrl.time_steps(K, *args, out=out)      # the waiting form
    wall_ms = (time.perf_counter() - t0) * 1e3
    print("TIME-BRACKETS time_steps: %d x %.4f ms on the device inside %.4f ms of host clock" % (K, ms, wall_ms))
    assert ms > 0.0
    assert K * ms <= wall_ms
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    each, _ = ctrl.time_steps_each(K, *args, out=out)
    wall_ms = (time.perf_counter() - t0) * 1e3
    print("TIME-BRACKETS time_steps_each: %s ms, sum %.4f inside %.4f ms of host clock" % (np.round(each, 4).tolist(), each.sum(), wall_ms))
    assert each.shape == (K,) and (each > 0.0).all()
    assert each.sum() <= wall_ms
    ctrl.close()


def test_statistics_of_timed_steps_equal_those_of_plain_steps():
    a, args, out = _setup()
    a.time_steps(K, *args, out=out)
    sa = a.stats()
    tau_a = out[0].cpu().numpy().copy()
    a.close()
    b, args, out = _setup()
    for _ in range(K):
        b.step(*args, out=out)
    sb = b.stats()
    tau_b = out[0].cpu().numpy()
    b.close()
    assert _exact(sa) == _exact(sb), (sa, sb)
    assert sa["ticks"] == K * N and sum(sa["mask_count"]) == K * N and sa["iters_sum"] > 0
    assert np.array_equal(tau_a, tau_b)
