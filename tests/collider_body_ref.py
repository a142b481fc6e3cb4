"""NumPy float64 restatement of the collider's rigid body (pbf_set_collider_body, include/pbf_hip.h), written from the text
of csrc/pbf_collider_body.hpp's head, operation for operation and in the order written there: R(q), the conversion of a
rotation matrix to a unit quaternion, one advance, and the parameter check.  Every value is a numpy.float64 scalar, so each
operation rounds once, as the header's double arithmetic does without contraction.

A Body is the parameters plus the state; advance() returns nothing and moves the state.  state_words() lays the state out
as struct pbf_collider_body_state does, for byte comparisons with the device's record and with the host program's lines."""
import numpy as np

F = np.float64


def rotation_of(q):
    """row-major R(q) of q = (w, x, y, z), nine float64"""
    w, x, y, z = (F(v) for v in q)
    one, two = F(1.0), F(2.0)
    return np.array([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                     two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                     two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], F)


def normalise(q):
    q = [F(v) for v in q]
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return np.array([v / n for v in q], F)


def quaternion_of(rot):
    """Shepperd's choice by the trace and the largest diagonal entry, then normalised"""
    r = [F(v) for v in np.asarray(rot, F).reshape(9)]
    one, two, four = F(1.0), F(2.0), F(4.0)
    tr = (r[0] + r[4]) + r[8]
    if tr > 0.0:
        s = two * np.sqrt(tr + one)
        q = [s / four, (r[7] - r[5]) / s, (r[2] - r[6]) / s, (r[3] - r[1]) / s]
    elif r[0] > r[4] and r[0] > r[8]:
        s = two * np.sqrt(((one + r[0]) - r[4]) - r[8])
        q = [(r[7] - r[5]) / s, s / four, (r[1] + r[3]) / s, (r[2] + r[6]) / s]
    elif r[4] > r[8]:
        s = two * np.sqrt(((one + r[4]) - r[0]) - r[8])
        q = [(r[2] - r[6]) / s, (r[1] + r[3]) / s, s / four, (r[5] + r[7]) / s]
    else:
        s = two * np.sqrt(((one + r[8]) - r[0]) - r[4])
        q = [(r[3] - r[1]) / s, (r[2] + r[6]) / s, (r[5] + r[7]) / s, s / four]
    return normalise(q)


PARAMS = ("mass", "inertia", "gain", "linear_damping", "angular_damping", "accel", "linear_factor", "angular_factor", "centre_min",
          "centre_max")


class Body:
    """the parameters as given and the state at rest in the start pose (rot is kept as given until the first advance)"""

    def __init__(self, mass, inertia=(1.0, 1.0, 1.0), rot=np.eye(3), centre=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0),
                 angular_velocity=(0.0, 0.0, 0.0), gain=0.49, accel=(0.0, 0.0, 0.0), linear_damping=0.0, angular_damping=0.0,
                 linear_factor=(1.0, 1.0, 1.0), angular_factor=(1.0, 1.0, 1.0), centre_min=(-np.inf,) * 3, centre_max=(np.inf,) * 3):
        v3 = lambda a: np.array(np.asarray(a, F).reshape(3), F)
        self.mass, self.gain, self.linear_damping, self.angular_damping = F(mass), F(gain), F(linear_damping), F(angular_damping)
        self.inertia, self.accel, self.linear_factor, self.angular_factor = v3(inertia), v3(accel), v3(linear_factor), v3(angular_factor)
        self.centre_min, self.centre_max = v3(centre_min), v3(centre_max)
        self.rot = np.array(np.asarray(rot, F).reshape(9), F)
        self.x, self.q, self.v, self.w = v3(centre), quaternion_of(rot), v3(velocity), v3(angular_velocity)
        self.impulse, self.angular = np.zeros(3), np.zeros(3)
        self.hits = self.steps = self.rejected = 0

    def kwargs(self):
        """the arguments of Solver.set_collider_body that place a device body in this one's CURRENT state"""
        d = {k: getattr(self, k) for k in PARAMS}
        d.update(rot=self.rot.reshape(3, 3), centre=self.x, velocity=self.v, angular_velocity=self.w)
        return d

    def pose(self):
        """(R (3, 3), x): what the next step's delta-p launches read, before the rounding to N"""
        return self.rot.reshape(3, 3).copy(), self.x.copy()

    def advance(self, dt, P, L, hits=0):
        dt = F(dt)
        P, L = [F(v) for v in P], [F(v) for v in L]
        x, q, v, w = self.x, self.q, self.v, self.w
        R = rotation_of(q)
        one, two = F(1.0), F(2.0)
        with np.errstate(all="ignore"):
            J = [-(self.gain * P[a]) / dt for a in range(3)]
            H = [-(self.gain * L[a]) / dt for a in range(3)]
            if not np.isfinite(J + H).all():
                J, H = [F(0.0)] * 3, [F(0.0)] * 3
                self.rejected += 1
            for a in range(3):
                v[a] = ((v[a] + dt * self.accel[a]) + J[a] / self.mass) * self.linear_factor[a] / (one + dt * self.linear_damping)
            k = [((R[b] * H[0] + R[3 + b] * H[1]) + R[6 + b] * H[2]) / self.inertia[b] for b in range(3)]
            for a in range(3):
                w[a] = ((w[a] + ((R[3 * a] * k[0] + R[3 * a + 1] * k[1]) + R[3 * a + 2] * k[2])) * self.angular_factor[a]) / \
                       (one + dt * self.angular_damping)
            for a in range(3):
                x[a] = x[a] + dt * v[a]
                if x[a] < self.centre_min[a]:
                    x[a], v[a] = self.centre_min[a], F(0.0)
                elif x[a] > self.centre_max[a]:
                    x[a], v[a] = self.centre_max[a], F(0.0)
            s = dt / two
            d = [-((w[0] * q[1] + w[1] * q[2]) + w[2] * q[3]), (w[0] * q[0] + w[1] * q[3]) - w[2] * q[2],
                 (w[1] * q[0] + w[2] * q[1]) - w[0] * q[3], (w[2] * q[0] + w[0] * q[2]) - w[1] * q[1]]
            self.q = normalise([q[c] + s * d[c] for c in range(4)])
        self.rot = rotation_of(self.q)
        self.impulse, self.angular, self.hits = np.array(P, F), np.array(L, F), int(hits)
        self.steps += 1
        return self

    def state_words(self):
        """the 31 64-bit words of struct pbf_collider_body_state, as bytes"""
        f = np.concatenate([self.rot, self.x, self.q, self.v, self.w, self.impulse, self.angular]).astype(F)
        return f.tobytes() + np.array([self.hits, self.steps, self.rejected], np.uint64).tobytes()


def params_ok(**kw):
    """the check of pbf_set_collider_body restated -> None when accepted, else the reason's key words"""
    import collider_pose_ref as PR
    b = dict(mass=1.0, inertia=(1.0,) * 3, gain=0.49, linear_damping=0.0, angular_damping=0.0, accel=(0.0,) * 3, linear_factor=(1.0,) * 3,
             angular_factor=(1.0,) * 3, centre_min=(-np.inf,) * 3, centre_max=(np.inf,) * 3, rot=np.eye(3), centre=(0.0,) * 3,
             velocity=(0.0,) * 3, angular_velocity=(0.0,) * 3)
    b.update(kw)
    flat = lambda names: np.concatenate([np.asarray(b[k], F).reshape(-1) for k in names])
    if not np.isfinite(flat(PARAMS[:8])).all() or np.isnan(flat(PARAMS[8:])).any():
        return "non-finite parameter"
    if not np.isfinite(flat(("velocity", "angular_velocity"))).all():
        return "non-finite start velocity"
    if not b["mass"] > 0:
        return "mass <= 0"
    if not (np.asarray(b["inertia"], F) > 0).all():
        return "inertia <= 0"
    if b["gain"] < 0:
        return "gain < 0"
    if b["linear_damping"] < 0 or b["angular_damping"] < 0:
        return "damping < 0"
    if not np.isin(flat(("linear_factor", "angular_factor")), (0.0, 1.0)).all():
        return "factor other than 0 or 1"
    if (np.asarray(b["centre_min"], F) > np.asarray(b["centre_max"], F)).any():
        return "centre_min > centre_max"
    if not PR.pose_ok(b["rot"], b["centre"]):
        return "pose"
    return None
