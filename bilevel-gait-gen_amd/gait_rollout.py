"""Closed-loop rollouts with the gait step (include/srbm_rti.h: srbm_gait_closed_loop_advance, srbm_plant_advance,
srbm_gait_get_line_search_result): the controller loop of controllers/mpc_controller.cpp:286-399 over the single-rigid-body plant, device resident
for a batch, with one step-log record per run.  A module of its own beside host.py: it calls through the library `host.declare` has typed."""
import ctypes as C

import numpy as np

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

# fields 58..63 of a step-log record written by srbm_gait_closed_loop_advance (every other entry leaves them 0)
GAIT_LOG_FIELDS = {'kind': 58, 'ready': 59, 'lp_status': 60, 'pred_red': 61, 'imin': 62, 'winner_cost': 63}
RUN_KINDS = {0: 'plain', 1: 'gradient', 2: 'line_search'}
LS_SIZE = 10


def gait_fields_from_log(record):
    """fields 58..63 of one step-log record [64] as a dict: kind (0 plain, 1 gradient and LP, 2 line search with a ready gradient) and its name,
    the ready flag after the run, lp_status and pred_red (kind 1, else 0), imin and the winner's cost / n (kind 2, else 0)"""
    r = np.asarray(record, dtype=np.float64)
    if r.shape != (64,):
        raise ValueError('one step-log record of 64 doubles expected, got shape %s' % (r.shape,))
    kind = int(r[GAIT_LOG_FIELDS['kind']])
    return dict(kind=kind, kind_name=RUN_KINDS[kind], ready=int(r[GAIT_LOG_FIELDS['ready']]), lp_status=int(r[GAIT_LOG_FIELDS['lp_status']]),
                pred_red=float(r[GAIT_LOG_FIELDS['pred_red']]), imin=int(r[GAIT_LOG_FIELDS['imin']]), winner_cost=float(r[GAIT_LOG_FIELDS['winner_cost']]))


class GaitRollout:
    """mpc: a host.BatchMPC with a plant state set; gait: the host.BatchGaitOptimizer that borrows it"""

    def __init__(self, mpc, gait):
        if gait.mpc is not mpc:
            raise ValueError('the gait optimiser belongs to another batch')
        self.mpc, self.gait, self.L = mpc, gait, mpc.L

    def advance(self, first_run_num, steps, gait_opt_freq, substeps=1, advance_time=False):
        """runs first_run_num .. first_run_num + steps - 1 (first_run_num >= 1: run r of instance b integrates its plant from (r - 1) p over p and
        solves at (r - 1) p + p, p its MPC period -- mpc_period.plant_set_period; the node step dt where none is set); gait_opt_freq counts runs; asynchronous"""
        self.mpc._chk(self.L.srbm_gait_closed_loop_advance(self.gait.g, int(first_run_num), int(steps), int(gait_opt_freq), int(substeps),
                                                           int(bool(advance_time))))

    def plant_advance(self, index, substeps=1, advance_time=False):
        """the plant half of closed-loop iteration `index` (from index p over p, p the MPC period of the instance: dt unless set), no solve:
        (state[batch][13], time[batch] = index p + p, ee[batch][4][3]) -- the inputs of the next solve"""
        m = self.mpc
        state, time, ee = np.zeros((m.batch, 13)), np.zeros(m.batch), np.zeros((m.batch, 4, 3))
        m._chk(self.L.srbm_plant_advance(m.h, int(index), int(substeps), int(bool(advance_time)), state.ctypes.data_as(_dp), time.ctypes.data_as(_dp),
                                         ee.ctypes.data_as(_dp)))
        return state, time, ee

    def line_search_result(self):
        """(imin[batch], costs[batch][10]) of the last line search; imin = -1 where the instance was not ready and took the plain update"""
        m = self.mpc
        imin, costs = np.zeros(m.batch, np.int32), np.zeros((m.batch, LS_SIZE))
        m._chk(self.L.srbm_gait_get_line_search_result(self.gait.g, imin.ctypes.data_as(_ip), costs.ctypes.data_as(_dp)))
        return imin, costs
