"""Posing by matrices (adypt_amd/csrc/device/pose.hpp) restated in numpy float32, whole arrays at a time: what adypt_pose_triangles and the device path
(Pose) are held against, bit for bit.  Written from the definition in include/adypt_hip.h and the header's opening comment, not from its loops: every
product and sum below is one binary32 operation on arrays, in the written order; numpy never contracts them."""
import numpy as np

from oracle import oracle_py as O

F = np.float32


def vertex_matrices(matrices, parts=None, joints=None, weights=None):
    """float32 [n, 3 (vertex), 3, 4]: parts — the part's matrix for all three vertices; skin — slots 0..3 in order, the first slot of non-zero weight
    gives w * B, every later one adds w * B, a slot of weight 0 is skipped (its index never used), all four 0 leave zeros"""
    B = np.ascontiguousarray(matrices, dtype=F).reshape(-1, 3, 4)
    if parts is not None:
        return np.repeat(B[np.asarray(parts, dtype=np.int64)][:, None], 3, axis=1)
    j = np.asarray(joints, dtype=np.int64).reshape(-1, 3, 4)
    w = np.ascontiguousarray(weights, dtype=F).reshape(-1, 3, 4)
    M = np.zeros(j.shape[:2] + (3, 4), dtype=F)
    started = np.zeros(j.shape[:2], dtype=bool)
    for k in range(4):
        use = w[..., k] != 0
        jk = np.where(use, j[..., k], 0)  # (a skipped slot's index may be anything: it selects nothing)
        term = (w[..., k][..., None, None] * B[jk]).astype(F)
        summed = (M + term).astype(F)
        M = np.where((use & ~started)[..., None, None], term, np.where((use & started)[..., None, None], summed, M))
        started |= use
    return M


def cofactors(M):
    """[..., 3, 3]: C[r][c] = A[r+1][c+1] * A[r+2][c+2] - A[r+1][c+2] * A[r+2][c+1], indices mod 3"""
    A = M[..., :3]
    C = np.zeros(A.shape, dtype=F)
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
            C[..., r, c] = ((A[..., r1, c1] * A[..., r2, c2]).astype(F) - (A[..., r1, c2] * A[..., r2, c1]).astype(F)).astype(F)
    return C


def pose(triangles, matrices, parts=None, joints=None, weights=None):
    """the posed TRI_DT triangles"""
    t = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1).copy()
    M = vertex_matrices(matrices, parts, joints, weights)              # [n, 3, 3, 4]
    p, nrm = t["p"].astype(F), t["n"].astype(F)                        # [n, 3 (vertex), 3 (axis)]
    x, y, z = (p[..., a][..., None] for a in range(3))                 # [n, 3, 1] against rows [n, 3, 3]
    with np.errstate(all="ignore"):
        t["p"] = ((((M[..., 0] * x).astype(F) + (M[..., 1] * y).astype(F)).astype(F) + (M[..., 2] * z).astype(F)).astype(F) + M[..., 3]).astype(F)
        C = cofactors(M)
        nx, ny, nz = (nrm[..., a][..., None] for a in range(3))
        q = (((C[..., 0] * nx).astype(F) + (C[..., 1] * ny).astype(F)).astype(F) + (C[..., 2] * nz).astype(F)).astype(F)
        len2 = (((q[..., 0] * q[..., 0]).astype(F) + (q[..., 1] * q[..., 1]).astype(F)).astype(F) + (q[..., 2] * q[..., 2]).astype(F)).astype(F)
        ok = (len2 > 0) & np.isfinite(len2)
        s = np.sqrt(np.where(ok, len2, F(1))).astype(F)
        t["n"] = np.where(ok[..., None], (q / s[..., None]).astype(F), q)
    return t


# ---- matrices the tests share ----
def rotation(axis, degrees, translation=(0.0, 0.0, 0.0)):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    return np.concatenate([R, np.asarray(translation, dtype=np.float64)[:, None]], axis=1).astype(F)


def identity():
    return np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)


def matrix_set(n, seed=3):
    """n matrices [n, 3, 4]: 0 a rotation with a translation, 1 a non-uniform scale, 2 a mirror, 3 zero, the rest gentle random affine maps (rotation
    times a scale in [0.8, 1.25] per axis, a small translation); fewer than 4 take the first ones"""
    rs = np.random.RandomState(seed)
    fixed = [rotation((0.3, 1.0, 0.2), 37.0, (0.5, -0.25, 1.0)),
             np.concatenate([np.diag([1.5, 0.5, 2.0]), np.array([[0.1], [0.2], [-0.3]])], axis=1).astype(F),
             np.concatenate([np.diag([-1.0, 1.0, 1.0]), np.array([[2.0], [0.0], [0.0]])], axis=1).astype(F),
             np.zeros((3, 4), dtype=F)]
    out = []
    for k in range(n):
        if k < len(fixed):
            out.append(fixed[k])
            continue
        m = rotation(rs.normal(size=3), rs.uniform(-40, 40), rs.normal(0, 0.5, size=3)).astype(np.float64)
        m[:, :3] = m[:, :3] @ np.diag(rs.uniform(0.8, 1.25, size=3))
        out.append(m.astype(F))
    return np.stack(out)


def parts_of(n, n_parts, seed=5):
    """int32 [n]: every part below min(n, n_parts) is used when n allows"""
    p = np.random.RandomState(seed).randint(0, n_parts, size=n).astype(np.int32)
    k = min(n, n_parts)
    p[:k] = np.arange(k)
    return p


def skin_of(n, n_joints, seed=9):
    """(joints uint16 [n, 3, 4], weights float32 [n, 3, 4]): per vertex one to four non-zero weights that sum to about 1, zero-weight slots in any
    position with indices far out of range, and a few vertices whose four weights are all 0"""
    rs = np.random.RandomState(seed)
    j = rs.randint(0, n_joints, size=(n, 3, 4))
    w = rs.uniform(0.05, 1.0, size=(n, 3, 4))
    w[rs.uniform(size=w.shape) < 0.4] = 0.0
    tot = w.sum(axis=-1, keepdims=True)
    w = np.where(tot > 0, w / np.where(tot > 0, tot, 1.0), 0.0).astype(F)
    j = np.where(w == 0, 65535 - rs.randint(0, 7, size=j.shape), j)
    return j.astype(np.uint16), w
