"""What the tests of the ground's terrain (test_wb_terrain_plant_host.py, test_gpu_wb_terrain_plant.py) share, built on wb_ground_plant_kit.py: a numpy
restatement of csrc/srbm_wb_terrain.hiph -- the patch search, the contact law along the patch normal in the statement order of include/srbm_rti.h
(every line one rounded operation, sums associated as written), the ground's 18-row solve with the forces in world components, the sub-steps with the
contact state carried along -- with the seeded inputs of the GPU tests, so that the host tests can check their branch margins without a GPU, and the
slope cases with their thresholds.  A plain module: no fixtures, nothing pytest collects."""
import numpy as np

import controller_rollout_kit as kit
import wb_ground_plant_kit as gk
import wb_torque_plant_kit as fd
from controller_rollout_kit import ik

INF = float('inf')
AIR, STICK, SLIP, CLAMP = gk.AIR, gk.STICK, gk.SLIP, gk.CLAMP
PATCHES, PATCH_DOUBLES = 8, 8
EMPTY = np.array([1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])         # x_min > x_max


def patch(x=(-INF, INF), y=(-INF, INF), z0=0.0, gx=0.0, gy=0.0, mu=0.6):
    return np.array([x[0], x[1], y[0], y[1], z0, gx, gy, mu], float)


def level_terrain(ground):
    """ground[batch][8] -> [batch][1][8]: per instance one unbounded level patch with the ground's z0 and mu (a ground without a plane, z0 = -inf,
    keeps that switch in the ground; its patch is at 0)"""
    ground = np.asarray(ground, float).reshape(-1, 8)
    return np.array([[patch(z0=g[0] if np.isfinite(g[0]) else 0.0, mu=g[3])] for g in ground])


def normal(gx, gy):
    """as the library forms it when the terrain is set"""
    gx, gy = float(gx), float(gy)
    s = np.sqrt((1.0 + gx * gx) + gy * gy)
    return -gx / s, -gy / s, 1.0 / s


def find_patch(p, terrain):
    """-> the LAST patch whose rectangle holds (p.x, p.y), -1: none; and the distance of the foot to the nearest bound of a patch that is not empty"""
    j, near = -1, INF
    for t, pt in enumerate(np.asarray(terrain, float).reshape(-1, 8)):
        if pt[0] <= p[0] <= pt[1] and pt[2] <= p[1] <= pt[3]:
            j = t
        if pt[0] <= pt[1] and pt[2] <= pt[3]:
            near = min(near, abs(p[0] - pt[0]), abs(p[0] - pt[1]), abs(p[1] - pt[2]), abs(p[1] - pt[3]))
    return j, near


def terrain_law(p, w, cs, gr, terrain):
    """foot position p[3], velocity w[3], state cs = (in_contact, anchor_x, anchor_y), ground gr[8] (its compliance; z0 = -inf: nothing under the
    instance), terrain[P][8] -> F[3] in world components, new cs[3], info: the branch, the patch found, whether the foot is (re-)anchored, the normal
    force and the margins of the decisions taken (delta; the unclamped normal force; n0 - lim relative to max(1, lim); the nearest patch bound)"""
    k_n, d_n, k_t, d_t = float(gr[1]), float(gr[2]), float(gr[4]), float(gr[5])
    px, py, pz = (float(x) for x in p)
    wx, wy, wz = (float(x) for x in w)
    j, near = find_patch(p, terrain) if gr[0] > -INF else (-1, INF)
    air = dict(branch=AIR, first=False, slip=False, patch=j, N=0.0, margins=[near])
    if j < 0:
        return np.zeros(3), np.zeros(3), air
    z0, gx, gy, mu = (float(x) for x in np.asarray(terrain, float).reshape(-1, 8)[j, 4:])
    nx, ny, nz = normal(gx, gy)
    hx = gx * px; hy = gy * py; h0 = z0 + hx; zp = h0 + hy; dz = zp - pz; delta = nz * dz
    if not delta > 0:
        air['margins'] = [abs(delta), near]
        return np.zeros(3), np.zeros(3), air
    first = cs[0] != 1 + j
    wn = (nx * wx + ny * wy) + nz * wz
    wtx = wx - wn * nx; wty = wy - wn * ny; wtz = wz - wn * nz
    ns = k_n * delta; nd = d_n * wn; n1 = ns - nd; N = max(0.0, n1)
    pbx = px + delta * nx; pby = py + delta * ny; pbz = pz + delta * nz
    if first:
        Ax, Ay, Az = pbx, pby, pbz
    else:
        Ax, Ay = float(cs[1]), float(cs[2])
        Az = (z0 + gx * Ax) + gy * Ay
    ex = px - Ax; ey = py - Ay; ez = pz - Az
    en = (nx * ex + ny * ey) + nz * ez
    etx = ex - en * nx; ety = ey - en * ny; etz = ez - en * nz
    dvx = d_t * wtx; dvy = d_t * wty; dvz = d_t * wtz
    t0x = -(k_t * etx) - dvx; t0y = -(k_t * ety) - dvy; t0z = -(k_t * etz) - dvz
    lim = mu * N
    nn = (t0x * t0x + t0y * t0y) + t0z * t0z
    n0 = np.sqrt(nn)
    if n0 <= lim:
        Tx, Ty, Tz, ax, ay, slip = t0x, t0y, t0z, Ax, Ay, False
    else:
        sc = lim / n0
        Tx = sc * t0x; Ty = sc * t0y; Tz = sc * t0z
        ax = pbx + (Tx + dvx) / k_t; ay = pby + (Ty + dvy) / k_t
        slip = True
    F = np.array([Tx + N * nx, Ty + N * ny, Tz + N * nz])
    info = dict(branch=CLAMP if not n1 > 0 else (SLIP if slip else STICK), first=bool(first), slip=slip, patch=j, N=N, n=np.array([nx, ny, nz]),
                T=np.array([Tx, Ty, Tz]), lim=lim, mu=mu, margins=[abs(delta), abs(n1), abs(n0 - lim) / max(1.0, lim), near])
    return F, np.array([1.0 + j, ax, ay]), info


def terrain_dynamics(model, q, v, tau, cs, gr, terrain):
    """the law on the four feet and M a = S' tau - C v - g + sum_i J_i' F_i -> sol[30] = (a, F[4][3]), cs_out[4][3], the four infos of the law"""
    robot = model.robot
    p = ik.forward_kinematics(model.legs, q)
    J = [robot.foot_jacobian_lwa(q, i) for i in range(4)]
    F, out, infos = np.zeros((4, 3)), np.zeros((4, 3)), []
    for i in range(4):
        F[i], out[i], info = terrain_law(p[i], J[i] @ v, np.asarray(cs, float).reshape(4, 3)[i], gr, terrain)
        infos.append(info)
    M, Cv, g = robot.dynamics_terms(q, v)
    r = -(Cv + g)
    r[6:] += tau
    for i in range(4):
        r = r + J[i].T @ F[i]
    return np.concatenate([np.linalg.solve(M, r), F.reshape(12)]), out, infos


def terrain_step(model, q, v, cs, control, off, kp, kd, lim, gr, terrain, h, S, k, mass, Ir_inv, push=None):
    """tick k of the plant on its terrain for one instance, as wb_ground_plant_kit.ground_step -> q+, v+, cs+, dict(pushed, clamped, deviation, sol,
    tau, infos of the last sub-step, history: the infos of every sub-step)"""
    q, v, cs = np.array(q, float), np.array(v, float), np.array(cs, float).reshape(4, 3)
    hs = h / S
    pushed = push is not None and kit.push_applies(k * h, h, push[0])
    history = []
    for s in range(S):
        tau, clamped, dev = fd.torque_law(control, q, v, kp, kd, lim, off)
        sol, cs, infos = terrain_dynamics(model, q, v, tau, cs, gr, terrain)
        history.append(infos)
        hv = hs * sol[:18]
        v = v + hv
        if s == S - 1 and pushed:
            imp = np.asarray(push[1], float)
            v[:3] = v[:3] + imp[:3] / mass
            v[3:6] = v[3:6] + Ir_inv @ imp[3:]
        q = ik.integrate(q, v, hs)
    return q, v, cs, dict(pushed=pushed, clamped=clamped, deviation=dev, sol=sol, tau=tau, infos=infos, history=history)


def tangent(rng, n):
    """a seeded unit vector in the plane with normal n"""
    a = rng.normal(size=3)
    a = a - (a @ n) * n
    return a / np.linalg.norm(a)


def plane_under(p, depth, gx, gy):
    """z0 of the plane with slopes (gx, gy) that lies `depth` above the foot p along its normal (below it for a negative depth)"""
    return p[2] + depth / normal(gx, gy)[2] - gx * p[0] - gy * p[1]


HALF = 0.05             # half the side of a foot's own patch: the feet of an instance are more than 0.2 m apart


def around(p, half=HALF):
    return dict(x=(p[0] - half, p[0] + half), y=(p[1] - half, p[1] + half))


# ---- the inputs of the law-and-solve GPU test ----
# per call and instance, per foot: (where, branch, state).  where: 'own' -- a patch of the foot's own; 'over' -- two patches hold the foot, the later
# one counts (the earlier one lies 3 cm higher with another slope and would push hard); 'none' -- no patch under the foot; 'empty' -- the only patch
# whose rectangle would hold the foot is an empty one (its bounds reversed, its plane 3 cm above the foot).  state: 'first' -- not in contact
# before; 'old' -- in contact with this patch, with an anchor; 'other' -- in contact with ANOTHER patch (its number and a far anchor stored):
# re-anchored as on a first touch
SOLVE_FEET = [[[('own', STICK, 'old'), ('own', SLIP, 'old'), ('own', CLAMP, 'old'), ('own', SLIP, 'first')],
               [('own', STICK, 'first'), ('own', CLAMP, 'first'), ('own', SLIP, 'other'), ('empty', AIR, 'old')],
               [('own', STICK, 'old'), ('over', SLIP, 'first'), ('none', AIR, 'old'), ('own', AIR, 'old')],
               [('own', SLIP, 'old'), ('own', STICK, 'first'), ('own', CLAMP, 'other'), ('own', STICK, 'other')]],
              [[('none', AIR, 'first'), ('own', CLAMP, 'old'), ('over', STICK, 'old'), ('own', SLIP, 'first')],
               [('own', SLIP, 'old'), ('own', AIR, 'first'), ('own', STICK, 'first'), ('own', CLAMP, 'first')],
               [('own', CLAMP, 'old'), ('own', STICK, 'other'), ('empty', AIR, 'first'), ('own', SLIP, 'other')],
               [('over', CLAMP, 'first'), ('own', SLIP, 'old'), ('none', AIR, 'old'), ('own', STICK, 'old')]]]
SOLVE_PATCHES = 4
SLOPES = [(0.1, -0.3), (-0.2, 0.4), (0.4, 0.1), (-0.3, -0.2), (0.25, 0.35), (-0.15, 0.1), (0.3, -0.4), (-0.4, 0.2)]
FRICTIONS = [0.4, 0.7, 0.55, 0.9, 0.3, 0.8, 0.65, 0.5]


def solve_cases(cfg, models, batch=4, seed=13):
    """-> a list of dict(q, v, tau, cs, ground, terrain [batch][SOLVE_PATCHES][8], want): want[b][foot] = (branch, (re-)anchored, patch found).
    Bases yawed and rolled; every foot with a patch has one of its own around it (slopes 0.1 .. 0.4 in both axes, a friction coefficient each),
    4 to 7 mm under the surface along the patch normal (5 mm above it for a foot in the air over a patch); the foot velocities and the stored
    states are set so that every foot takes the branch SOLVE_FEET names with a wide margin (asserted on the restatement by the host test)"""
    rng = np.random.default_rng(seed)
    q0 = np.array(cfg['init_config'], float)
    tb = np.asarray(cfg['torque_bounds'], float)
    calls = []
    for c, feet in enumerate(SOLVE_FEET):
        q = np.tile(q0, (batch, 1)); q[:, 7:] += rng.uniform(-0.05, 0.05, size=(batch, 12))
        q[:, :3] += rng.normal(size=(batch, 3)) * 0.1
        v = rng.normal(size=(batch, 18)) * 0.3
        tau = rng.uniform(-1, 1, size=(batch, 12)) * tb
        cs, ground, terrain, want = np.zeros((batch, 4, 3)), np.zeros((batch, 8)), np.zeros((batch, SOLVE_PATCHES, 8)), []
        for b in range(batch):
            yaw, roll = [(0.3, -0.2), (1.9, 0.15), (-2.6, 0.3), (0.7, -0.25)][(b + c) % 4]
            q[b, 3:7] = fd.quat_yaw_roll(yaw, roll)
            p = ik.forward_kinematics(models[b].legs, q[b])
            gr = gk.ground_params(0.123, k_n=3000.0 + 500.0 * b, d_n=40.0 + 10.0 * b, mu=0.05, k_t=2500.0 + 300.0 * b, d_t=25.0 + 5.0 * b)
            patches, wanted, mine = [], [], {}
            for i, (where, branch, state) in enumerate(feet[b]):
                gx, gy = SLOPES[(2 * b + i + 3 * c) % len(SLOPES)]
                mu = FRICTIONS[(b + 2 * i + c) % len(FRICTIONS)]
                depth = -0.005 if branch == AIR else 0.004 + 0.001 * ((i + b) % 4)
                if where == 'none':
                    wanted.append((AIR, False, -1))
                    continue
                if where == 'empty':
                    r = around(p[i])
                    patches.append(patch(x=r['x'][::-1], y=r['y'], z0=plane_under(p[i], 0.03, gx, gy), gx=gx, gy=gy, mu=mu))
                    wanted.append((AIR, False, -1))
                    continue
                if where == 'over':
                    patches.append(patch(z0=plane_under(p[i], 0.03, -gy, gx), gx=-gy, gy=gx, mu=1.0, **around(p[i], 0.8 * HALF)))
                mine[i] = len(patches)
                patches.append(patch(z0=plane_under(p[i], depth, gx, gy), gx=gx, gy=gy, mu=mu, **around(p[i])))
                wanted.append((branch, branch != AIR and state != 'old', mine[i]))
            while len(patches) < SOLVE_PATCHES:
                patches.append(EMPTY)
            assert len(patches) == SOLVE_PATCHES
            for i, (where, branch, state) in enumerate(feet[b]):
                far = [1.0 + (mine.get(i, 0) + 1) % SOLVE_PATCHES, p[i, 0] + 0.2, p[i, 1] - 0.3]          # another patch's number, an anchor far away
                if i not in mine or branch == AIR:
                    cs[b, i] = far if state != 'first' else 0.0
                    continue
                pt = patches[mine[i]]
                n = np.array(normal(pt[5], pt[6]))
                delta = n[2] * (pt[4] + pt[5] * p[i, 0] + pt[6] * p[i, 1] - p[i, 2])
                spring = gr[1] * delta
                along = tangent(rng, n)
                if branch == CLAMP:                            # rebounding along the normal: d_n w_n = 2 k_n delta
                    w = (2.0 * spring / gr[2]) * n + 0.2 * along
                    offset = 0.003 * along
                else:
                    wn = -0.1
                    limit = pt[7] * (spring - gr[2] * wn)
                    factor = 0.25 if branch == STICK else 3.0
                    if state == 'old':                         # T0 = -k_t offset - d_t w_t
                        w, offset = wn * n + 0.02 * along, along * (factor * limit / gr[4])
                    else:                                      # T0 = -d_t w_t
                        w, offset = wn * n + along * (factor * limit / gr[5]), np.zeros(3)
                v[b] = gk.set_foot_velocity(models[b], q[b], v[b], i, w)
                on_surface = p[i] + delta * n - offset
                cs[b, i] = [1.0 + mine[i], on_surface[0], on_surface[1]] if state == 'old' else (far if state == 'other' else 0.0)
            ground[b], terrain[b] = gr, np.array(patches)
            want.append(wanted)
        calls.append(dict(q=q, v=v, tau=tau, cs=cs, ground=ground, terrain=terrain, want=want))
    return calls


# ---- the inputs of the step-alone GPU test ----
TOUCH_DOWN, LIFT_OFF, SLIDE = (0, 0), (1, 1), (2, 2)       # (instance, foot): what happens to it in sub-step 2 of 3 in every round of step_cases
STEP_PATCHES = 5
SLIDE_EDGE = 1.5e-3             # the edge the sliding foot crosses lies this far ahead of it in x; it moves at 1 m/s, 3.3 mm per sub-step of three


def step_cases(cfg, models, h, batch=4, seed=79):
    """the inputs of the terrain-step GPU test, per round: wb_torque_plant_kit.step_cases' (k, q, v, control, status, pushes) with cs, ground and
    terrain [batch][STEP_PATCHES][8] added.  Every foot has a patch of its own around it with slopes of its own.  Foot TOUCH_DOWN starts 0.3 mm
    above its slope moving down along the normal at 1 m/s, foot LIFT_OFF 0.3 mm inside its slope moving up at 1 m/s, foot SLIDE stands 4 mm deep
    and moves along its slope at 1 m/s in x towards the edge of its patch SLIDE_EDGE away, behind which a patch with the same slopes, 0.5 mm
    higher and with a fifth of the friction begins: with S = 3 the three happen in sub-step 2 (asserted on the restatement by the host test).
    Of the other feet every other one is 2 mm inside its slope, with an anchor 1 mm away, the rest 2 mm above it"""
    rng = np.random.default_rng(seed)
    out = []
    for c in fd.step_cases(cfg, h, batch):
        q, v = c['q'].copy(), c['v'].copy()
        cs, ground, terrain = np.zeros((batch, 4, 3)), np.zeros((batch, 8)), np.tile(EMPTY, (batch, STEP_PATCHES, 1))
        for b in range(batch):
            p = ik.forward_kinematics(models[b].legs, q[b])
            ground[b] = gk.ground_params(-0.321, k_n=3000.0 + 500.0 * b, d_n=40.0 + 10.0 * b, mu=0.0, k_t=2500.0 + 300.0 * b, d_t=25.0 + 5.0 * b)
            for i in range(4):
                gx, gy = SLOPES[(b + 2 * i) % len(SLOPES)]
                mu = FRICTIONS[(2 * b + i) % len(FRICTIONS)]
                n = np.array(normal(gx, gy))
                r = around(p[i])
                if (b, i) == TOUCH_DOWN:
                    depth = -3e-4
                    v[b] = gk.set_foot_velocity(models[b], q[b], v[b], i, -1.0 * n + np.array([0.1, -0.05, 0.1 * gx - 0.05 * gy]))
                elif (b, i) == LIFT_OFF:
                    depth = 3e-4
                    v[b] = gk.set_foot_velocity(models[b], q[b], v[b], i, 1.0 * n + np.array([-0.05, 0.1, -0.05 * gx + 0.1 * gy]))
                elif (b, i) == SLIDE:
                    depth = 4e-3
                    v[b] = gk.set_foot_velocity(models[b], q[b], v[b], i, np.array([1.0, 0.0, gx]))
                    edge = p[i, 0] + SLIDE_EDGE
                    z0 = plane_under(p[i], depth, gx, gy)
                    terrain[b, 4] = patch(x=(edge, r['x'][1]), y=r['y'], z0=z0 + 5e-4, gx=gx, gy=gy, mu=0.2 * mu)
                    r = dict(x=(r['x'][0], edge), y=r['y'])
                    cs[b, i] = [1.0 + i, p[i, 0] - 1e-3, p[i, 1] + 1e-3]
                else:
                    depth = 2e-3 if (i + b) % 2 == 1 else -2e-3
                    if depth > 0:
                        cs[b, i] = [1.0 + i, p[i, 0] + 1e-3 * rng.normal(), p[i, 1] + 1e-3 * rng.normal()]
                terrain[b, i] = patch(z0=plane_under(p[i], depth, gx, gy), gx=gx, gy=gy, mu=mu, **r)
        d = dict(c); d.update(q=q, v=v, cs=cs, ground=ground, terrain=terrain)
        del d['contact']
        out.append(d)
    return out


# ---- the rollout ----
def rollout_terrain(world_q, legs, batch=4):
    """the terrain of the rollout test, [batch][2][8]: a base slope under the whole instance, 2 % in x and -1 % in y, 5 mm above the mean foot
    height of the plant's first configuration, and over it, with the same plane, a patch of low friction under the two left feet (y above the
    base's)"""
    out = np.zeros((batch, 2, 8))
    for b in range(batch):
        p = ik.forward_kinematics(legs, world_q[b])
        gx, gy = 0.02, -0.01
        z0 = float(np.mean(p[:, 2] - gx * p[:, 0] - gy * p[:, 1])) + 0.005
        out[b, 0] = patch(z0=z0, gx=gx, gy=gy, mu=0.7)
        out[b, 1] = patch(y=(world_q[b, 1], INF), z0=z0, gx=gx, gy=gy, mu=0.05)
    return out


def rollout_ground():
    """the compliance of the rollout's terrain (wb_ground_plant's rollout_ground); its z0 and mu are not used"""
    return gk.ground_params(0.0, k_n=5000.0, d_n=60.0, mu=0.0, k_t=3000.0, d_t=40.0)


# ---- physics on a slope ----
# The drop-and-settle case of wb_ground_plant_kit (its first instance, its SETTLE_* constants) turned as a whole about the world's y axis onto the
# plane z = tan(theta) x: the standing pose pitched by theta, 3 mm above the plane along its normal, constant control, no MPC.
#   (a) mu = SLOPE_MU_REST, well above tan(theta): it comes to rest, |v|_inf < V_REST and |sum N - m g cos(theta)| / (m g) < W_REST
#       (the restatement ends at |v|_inf SLOPE_REST_MEASURED[0] and a normal-force error of SLOPE_REST_MEASURED[1])
#   (b) mu = SLOPE_MU_SLIDE, below tan(theta): all four feet slip, and the base's downhill acceleration over the last 100 ticks (the second difference
#       of its position at ticks 200, 250, 300) is g (sin(theta) - mu cos(theta)) within SLOPE_SLIDE_BAND: three times the restatement's own
#       deviation from that closed form, SLOPE_SLIDE_MEASURED
SLOPE_THETA = 0.2
SLOPE_MU_REST, SLOPE_MU_SLIDE = 0.8, 0.05
SLOPE_MARKS = (200, 250, 300)
SLOPE_REST_MEASURED = (0.011, 0.0062)           # against V_REST 0.2 and W_REST 0.02
SLOPE_SLIDE_MEASURED = 0.0024                   # 1.4658 m/s^2 against the closed form's 1.4682
SLOPE_SLIDE_BAND = 3.0 * SLOPE_SLIDE_MEASURED
G = 9.81


def slide_closed_form(theta=SLOPE_THETA, mu=SLOPE_MU_SLIDE):
    return G * (np.sin(theta) - mu * np.cos(theta))


def slope_case(cfg, theta=SLOPE_THETA):
    """-> dict(model, bodies, q, v, control, kp, kd, lim, ground, terrain [2][1][8] for (a) and (b), weight, n, downhill)"""
    c = gk.settle_case(cfg)
    q = c['q'][0].copy()
    phi = -theta                                              # R_y(phi) takes e_z to the normal of z = tan(theta) x
    R = np.array([[np.cos(phi), 0.0, np.sin(phi)], [0.0, 1.0, 0.0], [-np.sin(phi), 0.0, np.cos(phi)]])
    q[:3] = R @ q[:3]
    q[3:7] = ik.quat_mul(np.array([0.0, np.sin(phi / 2), 0.0, np.cos(phi / 2)]), q[3:7])
    gx = np.tan(theta)
    terrain = np.array([[patch(gx=gx, mu=SLOPE_MU_REST)], [patch(gx=gx, mu=SLOPE_MU_SLIDE)]])
    return dict(model=c['models'][0], bodies=c['bodies'][0], q=q, v=np.zeros(18), control=c['control'][0], kp=c['kp'][0], kd=c['kd'][0], lim=c['lim'][0],
                ground=gk.ground_params(0.0, **dict(gk.SETTLE_GROUND, mu=0.0)), terrain=terrain, weight=float(c['weight'][0]),
                n=np.array(normal(gx, 0.0)), downhill=np.array([-np.cos(theta), 0.0, -np.sin(theta)]))


def slope_measures(v, sol, marks_q, case, theta=SLOPE_THETA):
    """-> |v|_inf, |sum N - m g cos(theta)| / (m g) from the last sub-step's (a, F), the downhill acceleration from the base positions at SLOPE_MARKS"""
    N = sol[18:].reshape(4, 3) @ case['n']
    x = [np.asarray(q)[:3] @ case['downhill'] for q in marks_q]
    dt = (SLOPE_MARKS[1] - SLOPE_MARKS[0]) * gk.SETTLE_H
    return float(np.abs(v).max()), float(abs(N.sum() - case['weight'] * np.cos(theta)) / case['weight']), float((x[2] - 2.0 * x[1] + x[0]) / (dt * dt))


def slope_restated(cfg, which):
    """case (a) (which = 0) or (b) (1) on the restatement -> v, cs, sol of the last sub-step, the configurations at SLOPE_MARKS, the last infos"""
    c = slope_case(cfg)
    ctrl = kit.Model(cfg)
    q, v, cs, marks = c['q'], c['v'], gk.NO_CONTACT, []
    for k in range(gk.SETTLE_TICKS):
        q, v, cs, info = terrain_step(c['model'], q, v, cs, c['control'], False, c['kp'], c['kd'], c['lim'], c['ground'], c['terrain'][which], gk.SETTLE_H,
                                      gk.SETTLE_S, k, ctrl.mass, ctrl.Ir_inv)
        if k + 1 in SLOPE_MARKS:
            marks.append(q.copy())
    return v, cs, info['sol'], marks, info['infos']
