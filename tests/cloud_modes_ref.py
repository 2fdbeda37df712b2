"""numpy restatement of the assignment pfmpe_cloud_modes defines (include/pfmpe.h), and the multi-modal cloud its tests
share.  numpy rounds every product and sum on its own, and the expressions below keep the operand order of
mode_dist / mode_assign (csrc/pfmpe_cloud.hip), so on inputs where no decision sits on a rounding the two agree exactly.
`assert_margin` is that condition on the inputs; it is evaluated with the numpy numbers alone."""
import functools

import numpy as np

MODE_NONE = 255
MARGIN = 1e-9
T_IDX = [3, 7, 11]
R_IDX = [0, 1, 2, 4, 5, 6, 8, 9, 10]

# the three hypotheses of the shared cloud: rotation vectors (rad) and translations (m)
SEED_TWISTS = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, -0.25, 0.1]])
SEED_TRANS = np.array([[0.0, 0.0, 1.0], [0.03, 0.0, 1.0], [0.0, 0.04, 1.02]])
ROT_SPREAD, TRANS_SPREAD = 0.08, 0.015
TRANS_SCALE, ROT_SCALE = 0.01, 0.05


def rodrigues(w):
    """Rotation matrices (n x 3 x 3) of rotation vectors w (n x 3)."""
    w = np.asarray(w, np.float64).reshape(-1, 3)
    th = np.sqrt((w * w).sum(axis=1))
    k = w / np.where(th > 0, th, 1.0)[:, None]
    Kx = np.zeros((len(w), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2] = -k[:, 2], k[:, 1]
    Kx[:, 1, 0], Kx[:, 1, 2] = k[:, 2], -k[:, 0]
    Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(th)[:, None, None] * Kx + (1 - np.cos(th))[:, None, None] * (Kx @ Kx)


def rows(R, t):
    """n x 12 rows (r00 r01 r02 t0 r10 ...) of rotations R (n x 3 x 3) and translations t (n x 3)."""
    return np.concatenate([R, t[:, :, None]], axis=2).reshape(len(R), 12)


def seeds(K=3, extra_seed=77):
    """K seed poses (K x 12): the three hypotheses above, then further ones scattered a few scales away."""
    tw, tr = SEED_TWISTS.copy(), SEED_TRANS.copy()
    if K > 3:
        rng = np.random.default_rng(extra_seed)
        tw = np.vstack([tw, rng.normal(0, 0.3, (K - 3, 3))])
        tr = np.vstack([tr, SEED_TRANS[0] + rng.normal(0, 0.04, (K - 3, 3))])
    return rows(rodrigues(tw[:K]), tr[:K])


@functools.lru_cache(maxsize=None)
def _cloud(N, gen_seed, through_fp32):
    rng = np.random.default_rng(gen_seed)
    which = rng.integers(0, 3, N)
    base = rodrigues(SEED_TWISTS)
    R = rodrigues(rng.normal(0, ROT_SPREAD, (N, 3))) @ base[which]
    t = SEED_TRANS[which] + rng.normal(0, TRANS_SPREAD, (N, 3))
    P = rows(R, t)
    if through_fp32:
        P = P.astype(np.float32).astype(np.float64)
    P.setflags(write=False)
    return P


def cloud(N, gen_seed=1, through_fp32=False):
    """N particles, each a member of one of the three hypotheses drawn at random, spread by 0.08 rad / 0.015 m about
    it: with the scales 0.01 m / 0.05 rad the modes overlap, so about 2 % of the particles are nearer to a
    neighbouring seed than to their own.  Cached and read-only."""
    return _cloud(int(N), int(gen_seed), bool(through_fp32))


def inv2(scale):
    return 1.0 / (scale * scale) if scale > 0 else 0.0


def distances(P, S, trans_scale=TRANS_SCALE, rot_scale=ROT_SCALE):
    """dist (N x K) of poses P (N x 12) to seeds S (K x 12), in the order the definition writes it."""
    P = np.asarray(P, np.float64).reshape(-1, 1, 12)
    S = np.asarray(S, np.float64).reshape(1, -1, 12)
    it2, ir2 = inv2(trans_scale), inv2(rot_scale)
    with np.errstate(invalid="ignore", over="ignore"):
        d = P[..., T_IDX] - S[..., T_IDX]
        d2 = d[..., 0] * d[..., 0]
        d2 = d2 + d[..., 1] * d[..., 1]
        d2 = d2 + d[..., 2] * d[..., 2]
        a, b = P[..., R_IDX], S[..., R_IDX]
        tr = a[..., 0] * b[..., 0]
        for k in range(1, 9):
            tr = tr + a[..., k] * b[..., k]
        return d2 * it2 + (3.0 - tr) * ir2


def assign(P, S, trans_scale=TRANS_SCALE, rot_scale=ROT_SCALE, max_dist=0.0):
    """(mode_of (N uint8), counts (K + 1 int64), best (N)) by the rule of the definition."""
    dist = distances(P, S, trans_scale, rot_scale)
    N, K = dist.shape
    best = np.full(N, np.inf)
    mode = np.full(N, MODE_NONE, dtype=np.uint8)
    for k in range(K):
        take = (dist[:, k] < best) & (dist[:, k] > -np.inf)
        best = np.where(take, dist[:, k], best)
        mode[take] = k
    if max_dist > 0:
        mode[~(best <= max_dist)] = MODE_NONE
    counts = np.array([(mode == k).sum() for k in range(K)] + [(mode == MODE_NONE).sum()], dtype=np.int64)
    return mode, counts, best


def assert_margin(P, S, trans_scale=TRANS_SCALE, rot_scale=ROT_SCALE, max_dist=0.0):
    """Every particle, no exclusions: its two smallest distances differ by more than a relative MARGIN, and with a
    gate its smallest distance is not within a relative MARGIN of max_dist.  Returns the smallest relative gap."""
    dist = distances(P, S, trans_scale, rot_scale)
    gap = np.inf
    if dist.shape[0] and dist.shape[1] >= 2:
        two = np.partition(dist, 1, axis=1)[:, :2]
        rel = (two[:, 1] - two[:, 0]) / np.abs(two[:, 1])
        gap = rel.min()
        assert gap > MARGIN, f"two seeds of an input particle are equally near (relative gap {gap:.3e})"
    if dist.shape[0] and max_dist > 0:
        assert np.all(np.abs(dist.min(axis=1) - max_dist) > MARGIN * max_dist), "an input particle sits on the gate"
    return gap
