"""numpy restatement of the cloud statistics defined in include/pfmpe.h (pfmpe_cloud_stats), vectorised over N.

The elementwise expressions keep the order of operations of the engine's pose_twist (csrc/pfmpe_cloud.hip), so that
the cancellations in D_R - D_R^T and t_i - D_R t_r round the same way on both sides and the two differ only by libm
rounding (sin, atan2) and by the order of the sums over particles."""
import numpy as np


def twists(P, ref, s_switch=1e-8, phi_switch=1e-4):
    """xi_i = [upsilon; omega] of T_i * T_ref^-1 for P (N x 12) about ref (12).  s_switch / phi_switch: the branch
    thresholds of the definition (the edge-case tests move them to evaluate the other branch's formula)."""
    P = np.asarray(P, np.float64).reshape(-1, 12)
    r = np.asarray(ref, np.float64).reshape(-1)[:12]
    same = np.all(P == r[None, :], axis=1)
    DR = np.empty((P.shape[0], 9))
    for i in range(3):
        for j in range(3):
            s = P[:, i * 4 + 0] * r[j * 4 + 0]
            s = s + P[:, i * 4 + 1] * r[j * 4 + 1]
            s = s + P[:, i * 4 + 2] * r[j * 4 + 2]
            DR[:, i * 3 + j] = s
    d = np.empty((P.shape[0], 3))
    for i in range(3):
        s = DR[:, i * 3 + 0] * r[3]
        s = s + DR[:, i * 3 + 1] * r[7]
        s = s + DR[:, i * 3 + 2] * r[11]
        d[:, i] = P[:, i * 4 + 3] - s
    a0 = 0.5 * (DR[:, 7] - DR[:, 5])
    a1 = 0.5 * (DR[:, 2] - DR[:, 6])
    a2 = 0.5 * (DR[:, 3] - DR[:, 1])
    s = np.sqrt((a0 * a0 + a1 * a1) + a2 * a2)
    c = 0.5 * (((DR[:, 0] + DR[:, 4]) + DR[:, 8]) - 1.0)
    phi = np.arctan2(s, c)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(s > s_switch, phi / s, 1.0 + (s * s) / 6.0)
        sh = np.sin(0.5 * phi)
        p2 = phi * phi
        k = np.where(phi >= phi_switch, (1.0 - (phi * np.sin(phi)) / (2.0 * ((2.0 * sh) * sh))) / p2,
                     1.0 / 12.0 + p2 / 720.0)
    w0, w1, w2 = f * a0, f * a1, f * a2
    c10 = w1 * d[:, 2] - w2 * d[:, 1]
    c11 = w2 * d[:, 0] - w0 * d[:, 2]
    c12 = w0 * d[:, 1] - w1 * d[:, 0]
    c20 = w1 * c12 - w2 * c11
    c21 = w2 * c10 - w0 * c12
    c22 = w0 * c11 - w1 * c10
    xi = np.stack([(d[:, 0] - 0.5 * c10) + k * c20, (d[:, 1] - 0.5 * c11) + k * c21, (d[:, 2] - 0.5 * c12) + k * c22,
                   w0, w1, w2], axis=1)
    xi[same] = 0.0
    return xi


def exp_map(xi):
    """exponentialMap (PE:2194-2226): twist [upsilon; omega] -> 3 x 4."""
    u, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R, V = np.eye(3), np.eye(3)
    if th != 0:
        O2 = O @ O
        R = np.eye(3) + O / th * np.sin(th) + O2 / (th * th) * (1 - np.cos(th))
        V = np.eye(3) + (1 - np.cos(th)) / (th * th) * O + (th - np.sin(th)) / (th * th * th) * O2
    return np.hstack([R, (V @ u)[:, None]])


def stats(P, w, ref):
    """The fields of pfmpe_cloud_out for poses P (N x 12), weights w (N, or None: unit) and the reference pose."""
    P = np.asarray(P, np.float64).reshape(-1, 12)
    N = P.shape[0]
    w = np.ones(N) if w is None else np.asarray(w, np.float64)
    r = np.asarray(ref, np.float64).reshape(-1)[:12]
    xi = twists(P, r)
    W = w.sum()
    if not W > 0:
        return {"n": N, "degenerate": 1, "wsum": W, "ess": 0.0, "mean_twist": np.zeros(6), "cov": np.zeros((6, 6)),
                "mean_pose": r.copy(), "max_trans": 0.0, "max_rot": 0.0}
    mu = (w[:, None] * xi).sum(axis=0) / W
    C = (xi.T * w[None, :]) @ xi / W - np.outer(mu, mu)
    E = exp_map(mu)
    R4 = np.vstack([r.reshape(3, 4), [0, 0, 0, 1]])
    pos = w > 0
    return {"n": N, "degenerate": 0, "wsum": W, "ess": W * W / (w * w).sum(), "mean_twist": mu, "cov": C,
            "mean_pose": (np.vstack([E, [0, 0, 0, 1]]) @ R4)[:3].reshape(12),
            "max_trans": np.sqrt((xi[pos, :3] ** 2).sum(axis=1)).max(),
            "max_rot": np.sqrt((xi[pos, 3:] ** 2).sum(axis=1)).max()}


def check(got, want, tol=1e-9):
    """|got - want| <= tol * max|want| for every array (cov: tol * the largest diagonal entry); n and the
    degenerate flag exactly."""
    assert got["n"] == want["n"] and got["degenerate"] == want["degenerate"], (got["n"], got["degenerate"])
    for k in ("wsum", "ess", "mean_twist", "cov", "mean_pose", "max_trans", "max_rot"):
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        scale = np.max(np.abs(np.diag(w))) if k == "cov" else np.max(np.abs(w))
        err = np.max(np.abs(g - w))
        print(f"cloud {k}: err {err:.3e} bound {tol * scale:.3e}")
        assert err <= tol * scale, (k, err, tol * scale)
