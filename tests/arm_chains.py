"""Serial chains that are NOT the Panda, and the problem constants that go with them -- shared by tests/test_gpu_planner.py (the
run-time chain code on the fused launch) and tests/test_gpu_gpmp_solve.py (the Gauss-Newton solve at six joints)."""
from tests import scenarios as SC


def arm7():
    """A 7-DoF arm that is NOT the Panda: its link lengths / offsets changed, another flange."""
    from stoch_gpmp_amd.robots.panda_chain import PANDA_CHAIN
    ch = [(nm, kind, tuple(rpy), list(xyz)) for nm, kind, rpy, xyz in PANDA_CHAIN]
    ch[0][3][2] = 0.36; ch[2][3][1] = -0.29; ch[3][3][0] = 0.07; ch[4][3][0] = -0.07; ch[4][3][1] = 0.41; ch[6][3][0] = 0.1
    ch[7][3][2] = 0.15                                   # a longer flange ...
    ch[8] = (ch[8][0], ch[8][1], (0.0, 0.0, 0.3), ch[8][3])          # ... turned differently
    return [(nm, kind, tuple(rpy), tuple(xyz)) for nm, kind, rpy, xyz in ch]


def arm6():
    """A 6-DoF arm (UR-like proportions): six revolute joints and a tool flange."""
    h = 1.57079632679
    return [("j1", "revolute", (0.0, 0.0, 0.0), (0.0, 0.0, 0.1625)), ("j2", "revolute", (h, 0.0, 0.0), (0.0, 0.0, 0.0)),
            ("j3", "revolute", (0.0, 0.0, 0.0), (-0.425, 0.0, 0.0)), ("j4", "revolute", (0.0, 0.0, 0.0), (-0.3922, 0.0, 0.1333)),
            ("j5", "revolute", (h, 0.0, 0.0), (0.0, -0.0997, 0.0)), ("j6", "revolute", (-h, 0.0, 0.0), (0.0, 0.0996, 0.0)),
            ("tool", "fixed", (0.0, 0.0, 0.0), (0.0, 0.0, 0.12))]


def arm_config(chain):
    n = sum(1 for j in chain if j[1] == "revolute")
    c = dict(SC.PANDA, n_dof=n)
    if n == 6:
        c.update(start_q=[0.1, -1.2, 1.4, -0.4, 0.8, 0.2], goal_q=[0.9, -0.7, 0.9, 0.3, 1.1, -0.4])
    return c, n
