"""The publication rule of the MPC computation latency on the host (no GPU): srbm_latency_publish_ticks_host through controller_rollout.publish_ticks
against a Python loop written from the rule of include/srbm_rti.h ("MPC computation latency") in np.float64, every rounded operation a statement of
its own, tick after tick from tick 1 with the published update number of every instance as its only state.  The library answers per update in
closed form through the two rule functions the publish kernel calls (csrc/srbm_mpc_latency.hiph), so the two are different programs.
Ticks of 10 ms as in tests/controller_rollout_kit.py; latencies that keep `due` at least 1 ms off every tick time, which the test asserts from its
own inputs: fl(k h) + L against fl(j h) never sits on a rounding tie."""
import numpy as np
import pytest

from srbm_loader import host
from srbm_loader.controller_rollout import publish_ticks

H = 0.01
MARGIN = 1e-3
LAST_TICK = 62          # the rollouts end before this tick


@pytest.fixture(scope='module')
def L():
    host.build()
    return host.lib()


def restated(first_tick, ticks, tpu, h, base, per, iters):
    """the header's rule, tick by tick -> tick[batch][n], overrun[batch][n], and the smallest |due - t_j| over the ticks an update could be published on"""
    B, n = iters.shape
    tick, over = np.full((B, n), -1, np.int32), np.zeros((B, n), np.int32)
    in_force = np.zeros(B, int)
    margin = np.inf
    for j in range(1, first_tick + ticks):
        e = (j - 1) // tpu
        if e > n:
            break
        time = np.float64(j) * np.float64(h)
        force = j % tpu == 0 and e >= 1
        for b in range(B):
            if not in_force[b] < e:
                continue
            t_start = np.float64(e * tpu) * np.float64(h)
            p = np.float64(per[b]) * np.float64(iters[b, e - 1])
            lat = np.float64(base[b]) + p
            due = t_start + lat
            margin = min(margin, abs(due - time))
            if due <= time or force:
                in_force[b] = e
                if j >= first_tick:
                    tick[b, e - 1] = j
                    over[b, e - 1] = int(not due <= time)
    return tick, over, margin


BASES = np.array([0.0, 0.012, 0.027, 0.080])
PER, PER_BASE = 1.7e-3, 0.4e-3
# iteration counts 5 .. 40 whose latency keeps the margin from every multiple of the tick (asserted again, on what the loop computes)
COUNTS = [i for i in range(5, 41) if all(abs(PER_BASE + PER * i - j * H) >= MARGIN + 1e-6 for j in range(8))]


@pytest.mark.parametrize('tpu', [1, 5])
def test_constant_latencies(L, tpu):
    n = LAST_TICK // tpu
    iters = np.zeros((4, n), np.int32) + 17          # (ignored: per_iteration = 0)
    for first, ticks in ((0, 36), (0, 1), (7, 20), (11, 1), (13, 9), (16, 19), (30, 30)):
        want_t, want_o, margin = restated(first, ticks, tpu, H, BASES, np.zeros(4), iters)
        assert margin >= MARGIN, (first, ticks, margin)
        got_t, got_o = publish_ticks(L, first, ticks, tpu, H, BASES, 0.0, iters)
        assert np.array_equal(got_t, want_t) and np.array_equal(got_o, want_o), (tpu, first, ticks, got_t, want_t, got_o, want_o)
    # ... and in words, the whole rollout: L = 0 is k + 1, 12 ms k + 2, 27 ms k + 3, 80 ms the forced tick k + period with the overrun flag
    t, o = publish_ticks(L, 0, LAST_TICK, tpu, H, BASES, 0.0, iters)
    k = tpu * np.arange(1, n + 1)
    inside = lambda x: np.where(x < LAST_TICK, x, -1)
    if tpu == 5:
        assert np.array_equal(t, [inside(k + 1), inside(k + 2), inside(k + 3), inside(k + 5)])
        assert np.array_equal(o, [0 * k, 0 * k, 0 * k, (k + 5 < LAST_TICK).astype(int)])
    else:       # every tick but the first is forced: everything is published at k + 1, late whatever is not due by then
        assert np.array_equal(t, [inside(k + 1)] * 4)
        assert np.array_equal(o, [0 * k, (k + 1 < LAST_TICK).astype(int), (k + 1 < LAST_TICK).astype(int), (k + 1 < LAST_TICK).astype(int)])


@pytest.mark.parametrize('tpu', [1, 5])
def test_latency_from_the_iterations(L, tpu):
    assert len(COUNTS) >= 24 and COUNTS[0] == 5 and COUNTS[-1] == 40
    n = LAST_TICK // tpu
    rng = np.random.default_rng(5)
    iters = rng.choice(COUNTS, size=(6, n)).astype(np.int32)
    iters[0, :len(COUNTS)] = COUNTS[:n]          # every count at least once
    base = np.full(6, PER_BASE)
    per = np.full(6, PER)
    for first, ticks in ((0, LAST_TICK), (9, 14), (23, 1), (31, 25)):
        want_t, want_o, margin = restated(first, ticks, tpu, H, base, per, iters)
        assert margin >= MARGIN, (first, ticks, margin)
        got_t, got_o = publish_ticks(L, first, ticks, tpu, H, base, per, iters)
        assert np.array_equal(got_t, want_t) and np.array_equal(got_o, want_o), (tpu, first, ticks)
    t, o = publish_ticks(L, 0, LAST_TICK, tpu, H, PER_BASE, PER, iters)
    if tpu == 5:        # the latency follows the work: every tick of a period is somebody's, and the long solves overrun
        assert {int(x) % 5 for x in t[t >= 0]} == {0, 1, 2, 3, 4} and 0 < o.sum() < (t >= 0).sum()
        assert np.all(o[t >= 0] == (PER_BASE + PER * iters[t >= 0] > 5 * H))


def test_refusals(L):
    iters = np.zeros((2, 3), np.int32)
    for bad, field in ((-1e-3, 'base'), (np.nan, 'base'), (np.inf, 'base')):
        with pytest.raises(RuntimeError, match='instance 1: ' + field):
            publish_ticks(L, 0, 10, 5, H, [0.0, bad], 0.0, iters)
    with pytest.raises(RuntimeError, match='instance 0: per_iteration'):
        publish_ticks(L, 0, 10, 5, H, 0.0, [-1.0, 0.0], iters)
    for args, msg in (((-1, 10, 5, H), 'first_tick'), ((0, -1, 5, H), 'ticks'), ((0, 10, 0, H), 'ticks_per_update'), ((0, 10, 5, 0.0), 'tick_dt'),
                      ((0, 10, 5, np.nan), 'tick_dt')):
        with pytest.raises(RuntimeError, match=msg):
            publish_ticks(L, *args, 0.0, 0.0, iters)
    iters[1, 2] = -1
    with pytest.raises(RuntimeError, match='instance 1, update 3'):
        publish_ticks(L, 0, 10, 5, H, 0.0, 0.0, iters)
