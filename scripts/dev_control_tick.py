"""The control tick of the whole batch, device resident, two ways:
  (a) chain   the three single entries bench.py's wbc segment times (srbm_get_targets_from_traj_dev, srbm_eval_trajectory_dev, srbm_qp_control_dev)
              with the contact forces stacked by torch between them
  (b) tick    srbm_control_tick_dev: two launches (the targets; then state reconstruction, stacking and the QP)
256 Config-B instances after the cold start, 200 ticks 1 ms apart, the two variants in turn, three runs each; medians.  Both draw the "measured"
state from the same seeded generator on the device, so they do the same work.
Every tick launch is under a time limit of its own (an alarm re-armed per tick: a launch or a wait that does not return ends the process).
Prints one JSON line."""
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from srbm_loader import host
from srbm_loader.control_tick import ControlTick
from srbm_loader.workloads import config_b_instance, instances

B, TICKS, WARM, DT, LIMIT_S = 256, 200, 3, 1e-3, 30.0
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 3          # (one run under a profiler)


def main():
    import torch
    signal.signal(signal.SIGALRM, signal.SIG_DFL)            # (the default action: the process ends, also from inside a driver call)
    cfg = host.load_config('a1_configuration')
    states, ees = instances(cfg, config_b_instance, B)
    signal.setitimer(signal.ITIMER_REAL, 300.0)
    mpc = host.BatchMPC.cold_start(cfg, states, ees)
    T = ControlTick(mpc)
    t0 = mpc.get_trajectory(0, 1)[0].init_time
    q_init = np.tile(np.array(cfg['init_config'], float), (B, 1))
    ext = torch.cuda.ExternalStream(mpc.stream())
    res = {'chain': [], 'tick': []}
    final, bad = {}, {}
    with torch.cuda.stream(ext):
        f64 = dict(dtype=torch.float64, device='cuda')
        i32 = dict(dtype=torch.int32, device='cuda')
        t_d = torch.zeros(B, **f64)
        q_d, v_d, f_d = torch.zeros((B, 19), **f64), torch.zeros((B, 18), **f64), torch.zeros((B, 4, 3), **f64)
        st_d, stq_d, st2_d = torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros((B, 2), **i32)
        ef_d, ep_d, con_d = torch.zeros((B, 12), **f64), torch.zeros((B, 12), **f64), torch.zeros((B, 4), **i32)
        ctl_d, sol_d = torch.zeros((B, 36), **f64), torch.zeros((B, 30), **f64)
        gen = torch.Generator(device='cuda')
        acc = torch.zeros(2, dtype=torch.int64, device='cuda')

        def measured():
            qm = q_d.clone(); qm[:, 7:] += 0.01 * torch.randn((B, 12), generator=gen, **f64)
            return qm, v_d + 0.01 * torch.randn((B, 18), generator=gen, **f64)

        def chain(k):
            t_d.fill_(t0 + DT * (k + 1))
            mpc.get_targets_from_traj_dev(t_d.data_ptr(), q_d.data_ptr(), v_d.data_ptr(), f_d.data_ptr(), st_d.data_ptr())
            mpc.eval_trajectory_dev(t_d.data_ptr(), ef_d.data_ptr(), ep_d.data_ptr(), con_d.data_ptr())
            order = torch.argsort((con_d == 0).to(torch.uint8), dim=1, stable=True)
            fd = (torch.take_along_dim(f_d, order[:, :, None], dim=1) * (torch.take_along_dim(con_d, order, dim=1) > 0)[:, :, None]).reshape(B, 12).contiguous()
            qm, vm = measured()
            mpc.qp_control_dev(qm.data_ptr(), vm.data_ptr(), con_d.data_ptr(), q_d.data_ptr(), v_d.data_ptr(), fd.data_ptr(), ctl_d.data_ptr(), sol_d.data_ptr(),
                               stq_d.data_ptr())
            acc[0] += (st_d != 0).sum(); acc[1] += ((stq_d & 255) > 1).sum()
            return fd, qm, vm

        def tick(k):
            # (the measured state of tick k is drawn around the targets of tick k - 1 here, around those of tick k in the chain: the same amount of
            #  work, not the same numbers)
            t_d.fill_(t0 + DT * (k + 1))
            qm, vm = measured()
            T.tick_dev(qm.data_ptr(), vm.data_ptr(), t_d.data_ptr(), ctl_d.data_ptr(), sol_d.data_ptr(), st2_d.data_ptr(), q_d.data_ptr(), v_d.data_ptr())
            acc[0] += (st2_d[:, 0] != 0).sum(); acc[1] += ((st2_d[:, 1] & 255) > 1).sum()
            return qm, vm

        variants = {'chain': chain, 'tick': tick}
        for run in range(RUNS):
            for name, fn in variants.items():
                gen.manual_seed(4242 + run)
                q_d.copy_(torch.tensor(q_init, **f64)); v_d.zero_()
                T.reset(q_init)
                keep = None
                for k in range(-WARM, 0):                    # warm-up: the ticks before the timed ones
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    keep = fn(k)
                mpc.synchronize(); acc.zero_()
                tb = time.perf_counter()
                for k in range(TICKS):
                    signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                    keep = fn(k)
                mpc.synchronize()
                res[name].append(1e3 * (time.perf_counter() - tb) / TICKS)
                signal.setitimer(signal.ITIMER_REAL, LIMIT_S)
                bad[name] = [int(x) for x in acc.cpu().numpy()]
                final[name] = ctl_d.cpu().numpy().copy()
    signal.setitimer(signal.ITIMER_REAL, 0)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({'batch': B, 'ticks': TICKS, 'runs': RUNS, 'ms_per_tick_runs': res, 'ms_per_tick_median': med,
                      'spread_ms': {k: float(max(v) - min(v)) for k, v in res.items()},
                      'targets_not_ok_and_qp_not_solved_last_run': bad,
                      'finite': bool(all(np.all(np.isfinite(v)) for v in final.values()))}))


if __name__ == '__main__':
    main()
