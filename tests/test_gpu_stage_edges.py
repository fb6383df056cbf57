"""Stage calls at their edges, HIP against the CPU oracle bit for bit: the 512-test matcher's tie
rules, vo_ransac_F / vo_ransac_run / vo_fit_F at the mask-word sizes, with more chunk threads than
matches, at other Sampson thresholds (the num / den < thr count form and its degenerate-denominator
rule) and probabilities (the per-probability bound table), and vo_pose over all four cheirality
candidates, its sign fixes and its degenerate exits.

Every case asserts on the oracle's own output that it is the regime it claims before it compares.
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle as O
from acs_visual_odometry_amd import Context
from acs_visual_odometry_amd.synth import KITTI_K, SceneSequence

pytestmark = pytest.mark.gpu
W, H, N = 320, 192, 500
VO_ERR_DEGENERATE_E = -10


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------
# matcher
# ---------------------------------------------------------------------------------------------

def _descriptors(rng, n):
    return rng.integers(0, 2**63, size=(n, 8), dtype=np.uint64)


def _match_sets():
    """{name: (queries, candidates)}.  Every crafted difference sits in tests 0..31 (word 0's low
    half), so the 32-test and the 512-test matcher both see it."""
    rng = np.random.default_rng(3)
    d = _descriptors(rng, 64)
    d2 = np.concatenate([d[:10], d[:10], d[10:20]])
    sets = {"ties%d" % i: s for i, s in enumerate([(d, d2), (d[:1], d2), (d, d2[:1]), (d[:5], d[:2]), (d2, d2)])}
    zeros = np.zeros((5, 8), np.uint64)
    ones = np.full((3, 8), 0xFFFFFFFFFFFFFFFF, np.uint64)
    sets["zeros_vs_ones"] = (zeros, ones)
    q = d[40:41].copy()
    near = q.copy()
    near[0, 0] ^= np.uint64(0b10110)                       # distance 3 at both widths
    far = q.copy()
    far[0, 0] ^= np.uint64(0xFFFF)                         # distance 16
    sets["equal_best_second"] = (q, np.concatenate([far, near, near, far]))
    sets["best_zero"] = (q, np.concatenate([far, q, near]))
    sets["best_second_zero"] = (q, np.concatenate([far, q, q]))
    # 70 queries against 2 .. 257 candidates: candidate j is query j % 70 with 1 + 7j % 5 + j // 70 of
    # its first 32 tests flipped, so a query has from no near candidate up to four at distances that
    # differ by one (accepted at 0.75 only where the best is below 3)
    qs = _descriptors(rng, 70)
    cs = qs[np.arange(257) % 70].copy()
    for j in range(257):
        for b in rng.choice(32, size=1 + (7 * j) % 5 + j // 70, replace=False):
            cs[j, 0] ^= np.uint64(1 << int(b))
    for nc in (2, 3, 64, 65, 257):
        sets["cands%d" % nc] = (qs, cs[:nc])
    return sets


@pytest.mark.parametrize("ratio", [0.75, 1.5])
@pytest.mark.parametrize("bits", [32, 512])
def test_match_crafted_sets(bits, ratio):
    """test_match_edge_cases' tie sets and crafted distance patterns through both matcher widths at
    ratio 0.75 and 1.5 (above 1 a query whose best and second-best distances are equal matches its
    first best candidate)."""
    sets = _match_sets()
    ref = {k: O.match(a, b, match_bits=bits, ratio=ratio) for k, (a, b) in sets.items()}
    # the regimes, on the oracle
    def dist(a, b):
        if bits == 32:
            return bin((int(a[0]) ^ int(b[0])) & 0xFFFFFFFF).count("1")
        return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))
    assert dist(*[s[0] for s in sets["zeros_vs_ones"]]) == bits
    q, c = sets["equal_best_second"]
    assert [dist(q[0], x) for x in c] == [16, 3, 3, 16]
    accept_equal = ratio > 1.0
    assert ref["zeros_vs_ones"].shape[0] == (5 if accept_equal else 0)
    assert ref["equal_best_second"].tolist() == ([[0, 1]] if accept_equal else [])
    assert ref["best_zero"].tolist() == [[0, 1]]                       # 0 < ratio * 3
    assert ref["best_second_zero"].tolist() == []                      # 0 < ratio * 0 never holds
    for nc in (2, 3, 64, 65, 257):
        m = ref["cands%d" % nc]
        assert (m.shape[0] == 70) if accept_equal else (0 < m.shape[0] < 70), (nc, m.shape)
    ctx = Context(W, H, max_kpts=N, match_bits=bits, ratio=ratio)
    try:
        for k, (a, b) in sets.items():
            m = ctx.match(a, b)
            assert m.shape == ref[k].shape, (k, m.shape, ref[k].shape)
            assert np.array_equal(m, ref[k]), k
        assert ctx.match(sets["ties0"][0][:0], sets["ties0"][0]).shape[0] == 0
        assert ctx.match(sets["ties0"][0], sets["ties0"][0][:0]).shape[0] == 0
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# RANSAC and fit
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pts_sets():
    """Matched points of two 320 x 192 scene frames ("all"), and 500 of them (tiled, the copies
    moved by whole pixels)."""
    seq = SceneSequence(W, H, nframes=2, step=0.05)
    frames = seq.frames()
    cfg = O.config(W, H, max_kpts=N)
    k0, d0, _ = O.extract(frames[0], cfg)
    k1, d1, _ = O.extract(frames[1], cfg)
    m = O.match(d0, d1)
    pts = np.concatenate([k0[m[:, 0]], k1[m[:, 1]]], axis=1).astype(np.float64)
    assert 129 < pts.shape[0] < N, pts.shape
    reps = -(-N // pts.shape[0])
    rng = np.random.default_rng(17)
    jit = rng.integers(-2, 3, size=(reps * pts.shape[0], 4)).astype(np.float64)
    jit[:pts.shape[0]] = 0.0
    big = (np.tile(pts, (reps, 1)) + jit)[:N]
    return pts, np.ascontiguousarray(big)


def _sizes(pts_all):
    return [8, 9, 15, 63, 64, 65, 128, 129, pts_all.shape[0], N]


def _assert_ransac(g, r, tag):
    assert g["n_evaluated"] == r["n_evaluated"], tag
    assert g["best_k"] == r["best_k"], tag
    assert np.array_equal(g["counts"], r["counts"]), tag
    assert g["n_inl"] == r["n_inl"], tag
    assert np.array_equal(g["inliers"], r["inliers"]), tag
    assert g["fitted"] == r["fitted"], tag
    if r["fitted"]:
        assert np.array_equal(g["F"], r["F"]), tag


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("T", [1, 8, 64])
def test_ransac_sizes_bit_exact(T, rng_mode, pts_sets):
    """vo_ransac_F at m = 8, 9, the 64-bit mask-word edges, every match and max_kpts, with 1, 8 and 64
    chunk threads.  T > m scores no match at all (quirk 7: T * floor(m / T) = 0): every count is 0,
    no hypothesis is best, the bound stays at its initial 1176."""
    pts_all, pts_big = pts_sets
    sizes = _sizes(pts_all) if rng_mode == 0 else [8, 65, pts_all.shape[0]]
    ctx = Context(W, H, max_kpts=N, ransac_chunk_threads=T, rng_mode=rng_mode)
    try:
        some_fit = False
        for m in sizes:
            pts = pts_big[:m]
            r = O.ransac(pts, T=T, seed=100 + m, rng_mode=rng_mode)
            if T > m:
                assert (r["best_k"], r["n_evaluated"], r["fitted"], r["n_inl"]) == (-1, 1176, 0, 0), (m, r)
                assert not r["counts"].any()
            elif m >= 63:
                assert r["fitted"] == 1 and r["n_inl"] >= 8, (m, r["n_inl"])
            some_fit |= bool(r["fitted"])
            _assert_ransac(ctx.ransac(pts, 100 + m), r, (T, rng_mode, m))
        assert some_fit
        assert ctx.device_errors() == 0
    finally:
        ctx.close()


DBL_MAX = 1.7976931348623157e308


@pytest.fixture(scope="module")
def deg_set():
    """64 correspondences of a pure translation (0.3 px noise) of which three are replaced by one
    duplicated pair: the two epipoles of the hypothesis k that wins at threshold 0.25.  F_k x and
    F_k^T x' vanish there, so that hypothesis' Sampson denominator is below 1e-12 and its error is
    DBL_MAX for the three -- inliers under an infinite threshold only.  -> (pts, dup indices, k)"""
    rng = np.random.default_rng(23)
    _, t, X, _ = _motion_case(rng, KITTI_K, n=64)
    pts = np.concatenate([_project(KITTI_K, X), _project(KITTI_K, X + t)], axis=1) + rng.normal(0.0, 0.3, (64, 4))
    r = O.ransac(pts, thr=0.25, T=8, seed=9)
    k = r["best_k"]
    s8 = O.sample8(9, k, 64)
    Fk = O.fit_F8(pts, s8)
    U, _, Vt = np.linalg.svd(Fk)
    e1, e2 = Vt[2] / Vt[2, 2], U[:, 2] / U[2, 2]
    dup = [j for j in range(64) if j not in set(s8) and j not in set(r["inliers"])][:3]
    assert len(dup) == 3
    pts[dup] = [e1[0], e1[1], e2[0], e2[1]]
    pts = np.ascontiguousarray(pts)
    # the regime, on the oracle: hypothesis k is unchanged (the three are not in its sample), their
    # error under it is DBL_MAX, it still wins at every small threshold without them, and its count
    # differs between the largest finite threshold and +inf by exactly the three
    assert np.array_equal(O.fit_F8(pts, s8), Fk)
    assert [O.sampson(Fk, pts[j]) for j in dup] == [DBL_MAX] * 3
    for thr in (1e-3, 0.25, 3.84):
        rr = O.ransac(pts, thr=thr, T=8, seed=9)
        assert rr["best_k"] == k and rr["n_inl"] >= 8 and not set(dup) & set(rr["inliers"]), (thr, rr["best_k"])
    big, inf = O.ransac(pts, thr=1e6, T=8, seed=9), O.ransac(pts, thr=math.inf, T=8, seed=9)
    assert inf["counts"][k] == 64 and big["counts"][k] == 61
    assert set(dup) <= set(inf["inliers"])
    return pts, dup, k


@pytest.fixture(scope="module")
def ctx_stage():
    c = Context(W, H, K=KITTI_K, max_kpts=N)
    yield c
    c.close()


def _assert_run(g, r, tag):
    assert g["fitted"] == r["fitted"], tag
    assert g["n_inl"] == r["n_inl"], tag
    assert g["n_evaluated"] == r["n_evaluated"], tag
    assert np.array_equal(g["inliers"], r["inliers"]), tag
    if r["fitted"]:
        assert np.array_equal(g["F"], r["F"]), tag
    else:
        assert g["F"] is None, tag


THRESHOLDS = [0.0, 1e-3, 0.25, 3.84, 1e6, math.inf]


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_ransac_run_thresholds_bit_exact(thr, pts_sets, deg_set, ctx_stage):
    """vo_ransac_run's own threshold: every value but 1.0 counts by num / den < thr.  On the oracle the
    inlier count grows with the threshold; 0 accepts nothing, +inf everything scored, including the
    degenerate-denominator matches (deg_set) that no finite threshold accepts."""
    pts_all, pts_big = pts_sets
    deg, dup, _ = deg_set
    m = pts_all.shape[0]
    ref = {t: O.ransac(pts_all, thr=t, T=8, seed=7) for t in THRESHOLDS}
    n = [ref[t]["n_inl"] for t in THRESHOLDS]
    assert n[0] == 0 and n == sorted(n) and n[1] < n[3] and n[-1] == (m // 8) * 8, n
    assert ref[0.0]["n_evaluated"] == 1176 and ref[0.0]["fitted"] == 0
    for pts, seed, tag in ((pts_all, 7, "all"), (pts_big, 8, "500"), (deg, 9, "degenerate")):
        r = O.ransac(pts, thr=thr, T=8, seed=seed)
        g = ctx_stage.ransac_run(pts, probability=0.99, sampson_thr=thr, num_threads=8, seed=seed)
        _assert_run(g, r, (thr, tag))
    assert ctx_stage.device_errors() == 0


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_ransac_F_context_threshold_bit_exact(thr, pts_sets, deg_set):
    """The same thresholds as the context's own sampson_thr, through vo_ransac_F: the per-hypothesis
    counts too, so the degenerate-denominator rule is compared on every hypothesis."""
    pts_all, _ = pts_sets
    deg = deg_set[0]
    ctx = Context(W, H, max_kpts=N, sampson_thr=thr)
    try:
        for pts, seed in ((pts_all, 7), (deg, 9)):
            r = O.ransac(pts, thr=thr, T=8, seed=seed)
            _assert_ransac(ctx.ransac(pts, seed), r, (thr, seed))
        assert ctx.device_errors() == 0
    finally:
        ctx.close()


def test_ransac_run_probabilities_and_table_cache(pts_sets, ctx_stage):
    """vo_ransac_run's probability: the initial bound (thr = 0: no hypothesis ever has an inlier, so
    n_evaluated is that bound) and the bound table of the call's probability (thr = 1: the bound after
    each new best comes from the table), with 0.999, 0.5, 0.999 in turn on one context so the cached
    table is replaced and rebuilt; and more hypotheses than the context holds is VO_ERR_CAPACITY."""
    pts_all, pts_big = pts_sets
    order = [0.999, 0.5, 0.999, 0.99, 0.5]
    bound = {0.5: 177, 0.99: 1176, 0.999: 1764}
    for p in order:
        r = O.ransac(pts_all, prob=p, thr=0.0, T=8, seed=3)
        assert r["n_evaluated"] == bound[p] and r["n_inl"] == 0
        _assert_run(ctx_stage.ransac_run(pts_all, probability=p, sampson_thr=0.0, num_threads=8, seed=3), r, (p, 0.0))
    evaluated = {}
    for p in order:
        for pts, tag in ((pts_all, "all"), (pts_big, "500")):
            r = O.ransac(pts, prob=p, thr=1.0, T=8, seed=4)
            assert r["fitted"] == 1 and r["n_evaluated"] < bound[p]      # the table lowered the bound
            evaluated[(p, tag)] = r["n_evaluated"]
            _assert_run(ctx_stage.ransac_run(pts, probability=p, sampson_thr=1.0, num_threads=8, seed=4), r, (p, tag))
    assert len({evaluated[(p, "500")] for p in bound}) == 3, evaluated   # each probability its own bound
    # 0.9999 needs 2353 hypotheses, the context has 2000 slots
    assert O.lib().voo_ransac_maxit_initial(0.9999) > 2000
    with pytest.raises(RuntimeError, match=r"capacity.*\(-4\)"):
        ctx_stage.ransac_run(pts_all, probability=0.9999, sampson_thr=1.0, num_threads=8, seed=4)
    r = O.ransac(pts_all, prob=0.999, thr=1.0, T=8, seed=5)
    _assert_run(ctx_stage.ransac_run(pts_all, probability=0.999, sampson_thr=1.0, num_threads=8, seed=5), r, "after")
    assert ctx_stage.device_errors() == 0


@pytest.mark.parametrize("T", [1, 3, 64])
def test_ransac_run_num_threads_bit_exact(T, pts_sets, ctx_stage):
    pts_all, pts_big = pts_sets
    m = pts_all.shape[0]
    dropped = m - (m // T) * T
    assert dropped == {1: 0}.get(T, dropped) and (T == 1 or dropped > 0), (m, T, dropped)
    for pts, thr in ((pts_all, 1.0), (pts_all, 0.25), (pts_big, 3.84), (pts_big[:40], 0.25)):
        r = O.ransac(pts, thr=thr, T=T, seed=11)
        if T > pts.shape[0]:
            assert (r["n_evaluated"], r["fitted"], r["n_inl"]) == (1176, 0, 0)
        else:
            assert r["inliers"].size == 0 or r["inliers"].max() < (pts.shape[0] // T) * T
        _assert_run(ctx_stage.ransac_run(pts, probability=0.99, sampson_thr=thr, num_threads=T, seed=11), r, (T, thr))
    assert ctx_stage.device_errors() == 0


def _fit_sets(pts_big):
    sets = {"n%d" % n: pts_big[:n] for n in (8, 9, 64, 65, N)}
    x = np.arange(40, dtype=np.float64)
    sets["collinear"] = np.stack([20 + 5 * x, 30 + 3 * x, 24 + 5 * x, 31 + 3 * x], axis=1)
    sets["three_points"] = np.tile(pts_big[:3], (10, 1))
    sets["zero_motion"] = np.concatenate([pts_big[:40, :2], pts_big[:40, :2]], axis=1)
    return sets


@pytest.mark.parametrize("name", ["n8", "n9", "n64", "n65", "n500", "collinear", "three_points", "zero_motion"])
def test_fit_F_bit_exact(name, pts_sets, ctx_stage):
    """vo_fit_F on 8 .. max_kpts correspondences and on three sets without a unique F (collinear
    points, three distinct points, no motion): the oracle's solver still returns a finite F there, and
    the device must return the same one."""
    pts = np.ascontiguousarray(_fit_sets(pts_sets[1])[name])
    Fr = O.fit_F(pts, np.arange(pts.shape[0], dtype=np.int32))
    assert np.isfinite(Fr).all() and np.abs(Fr).max() > 0
    F = ctx_stage.fit_F(pts)
    assert np.array_equal(F, Fr), (name, F, Fr)
    assert ctx_stage.device_errors() == 0


# ---------------------------------------------------------------------------------------------
# pose
# ---------------------------------------------------------------------------------------------

def _pose_rc(ctx, F, p1, p2, scale=1.0):
    """vo_pose's return code with its outputs (Context.pose raises on the degenerate code)."""
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
    p1 = np.ascontiguousarray(p1, dtype=np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, dtype=np.float32).reshape(-1, 2)
    R, t, cnt = np.zeros(9), np.zeros(3), np.zeros(4, np.int32)
    rc = ctx.lib.vo_pose(ctx.h, _p(F), _p(p1), _p(p2), p1.shape[0], scale, _p(R), _p(t), _p(cnt))
    return rc, R.reshape(3, 3), t, cnt


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def _rodrigues(axis, angle):
    A = _skew(axis / np.linalg.norm(axis))
    return np.eye(3) + math.sin(angle) * A + (1.0 - math.cos(angle)) * (A @ A)


def _project(K, X):
    x = X @ K.T
    return x[:, :2] / x[:, 2:3]


def _motion_case(rng, K, n=24, depth=(6.0, 30.0)):
    """A motion X2 = R X1 + t (|t| = 1, up to 0.4 rad about a random axis) and n points in front of
    both cameras: (R, t, X1, X2)."""
    while True:
        t = rng.standard_normal(3)
        t /= np.linalg.norm(t)
        R = _rodrigues(rng.standard_normal(3), rng.uniform(0.0, 0.4))
        z = rng.uniform(depth[0], depth[1], n)
        X = np.stack([z * rng.uniform(-0.6, 0.6, n), z * rng.uniform(-0.2, 0.2, n), z], axis=1)
        X2 = X @ R.T + t
        if X2[:, 2].min() > 1.0:
            return R, t, X, X2


def _fundamental(K, R, t):
    Ki = np.linalg.inv(K)
    return Ki.T @ (_skew(t) @ R) @ Ki


def pose_battery(K=KITTI_K, ncases=60, seed=5):
    """ncases // 3 motions, each as three correspondence sets of the same F or its transpose:
    "front" (the points in front of both cameras), "mirror" (the cloud mirrored through camera 1's
    centre, behind both cameras: the images of the motion (R, -t)), "swap" (p1 and p2 exchanged with
    F^T: the inverse motion).  -> [(kind, F, p1, p2, R_true, t_true)]"""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(ncases // 3):
        R, t, X, X2 = _motion_case(rng, K)
        F = _fundamental(K, R, t)
        p1, p2 = _project(K, X), _project(K, X2)
        cases.append(("front", F, p1, p2, R, t))
        Xm = -X
        cases.append(("mirror", F, _project(K, Xm), _project(K, Xm @ R.T + t), R, t))
        cases.append(("swap", F.T, p2, p1, R.T, -R.T @ t))
    return [(k, F, p1.astype(np.float32), p2.astype(np.float32), R, t) for k, F, p1, p2, R, t in cases]


def _assert_pose(ctx, F, K, p1, p2, scale=1.0, tag=None):
    rc_r, Rr, tr, cr = O.pose(F, K, p1, p2, scale)
    rc, R, t, c = _pose_rc(ctx, F, p1, p2, scale)
    assert (rc != 0) == (rc_r != 0) and rc in (0, VO_ERR_DEGENERATE_E), (tag, rc, rc_r)
    if rc_r == 0:
        assert np.array_equal(c, cr), (tag, c, cr)
        assert np.array_equal(R, Rr), (tag, R, Rr)
        assert np.array_equal(t, tr), (tag, t, tr)
    return rc_r, Rr, tr, cr


def test_pose_every_candidate_bit_exact(ctx_stage):
    """vo_pose on 60 correspondence sets of known motions: R, t and the four positive-depth counts equal
    the oracle's.  On the oracle, each of the four cheirality candidates wins somewhere in the battery,
    numpy's SVD of the normalised E has det(U) < 0 and det(Vt) < 0 each somewhere, and for the
    in-front sets the recovered motion is the generating one (largest entry error of R and t seen on
    the oracle: 6.0e-16; the bound 1e-9 guards the construction of the cases, not rounding -- a wrong
    candidate is off by 0.1 or more)."""
    K = KITTI_K
    winners, detU, detVt, worst = set(), set(), set(), 0.0
    for i, (kind, F, p1, p2, Rt, tt) in enumerate(pose_battery(K)):
        rc, R, t, cnt = _assert_pose(ctx_stage, F, K, p1, p2, 1.0, (i, kind))
        assert rc == 0
        winners.add(int(np.argmax(cnt)))                   # first maximum, as getPose
        E = K.T @ F @ K
        U, _, Vt = np.linalg.svd(E / np.linalg.norm(E))
        detU.add(np.linalg.det(U) < 0)
        detVt.add(np.linalg.det(Vt) < 0)
        if kind in ("front", "swap"):
            assert cnt.max() == p1.shape[0] and sorted(cnt)[-2] < cnt.max(), (i, kind, cnt)
            err = max(np.abs(R - Rt).max(), np.abs(t - tt).max())
            worst = max(worst, err)
            assert err <= 1e-9, (i, kind, err)
        else:
            assert cnt.max() > 0, (i, kind, cnt)
    assert winners == {0, 1, 2, 3}, winners
    assert detU == {False, True} and detVt == {False, True}
    assert ctx_stage.device_errors() == 0


def test_pose_no_parallax_and_ties(ctx_stage):
    """p2 == p1: no triangulation has a positive depth in both cameras, the four counts are 0 and the
    first candidate wins.  And a four-way tie with nonzero counts: three correspondences from each of
    the four motions that share one E (R or its twisted pair, t or -t), near the baseline where points
    can lie in front of both cameras of a twisted pair -- again the first candidate wins."""
    K = KITTI_K
    rng = np.random.default_rng(8)
    R, t, X, X2 = _motion_case(rng, K)
    F = _fundamental(K, R, t)
    p1 = _project(K, X).astype(np.float32)
    # F of a pure translation: with p2 == p1 the two rays of a correspondence are parallel under
    # R = I (a point at infinity: |w| < 1e-6, skipped), and the twisted pair puts none in front of both
    rc, _, _, cnt = _assert_pose(ctx_stage, _fundamental(K, np.eye(3), t), K, p1, p1, 1.0, "no parallax")
    assert rc == 0 and cnt.tolist() == [0, 0, 0, 0]
    Rtw = _rodrigues(t, math.pi) @ R                       # the twisted pair: [t]x Rtw = -[t]x R
    q1, q2 = [], []
    for Rm, tm in ((R, t), (R, -t), (Rtw, t), (Rtw, -t)):
        got = 0
        while got < 3:
            Xn = rng.uniform(-2.0, 2.0, 3)
            Xn2 = Rm @ Xn + tm
            if Xn[2] > 0.2 and Xn2[2] > 0.2:
                q1.append(_project(K, Xn[None])[0])
                q2.append(_project(K, Xn2[None])[0])
                got += 1
    q1, q2 = np.array(q1, np.float32), np.array(q2, np.float32)
    rc, Rr, tr, cnt = _assert_pose(ctx_stage, F, K, q1, q2, 1.0, "tie")
    assert rc == 0 and cnt.tolist() == [3, 3, 3, 3], cnt
    first = O.pose(F, K, q1[:3], q2[:3])                   # only the first group: its motion wins alone
    assert first[0] == 0


@pytest.mark.parametrize("scale", [0.0, 1e-3, 1.0, 37.5])
def test_pose_scales(scale, ctx_stage):
    K = KITTI_K
    for i, (kind, F, p1, p2, Rt, tt) in enumerate(pose_battery(K, ncases=6, seed=9)):
        rc, R, t, _ = _assert_pose(ctx_stage, F, K, p1, p2, scale, (i, kind, scale))
        assert rc == 0
        assert abs(np.linalg.norm(t) - scale) <= 1e-12 * max(scale, 1.0)


@pytest.mark.parametrize("n", [8, 9, 64, 65, N])
def test_pose_point_counts(n, ctx_stage):
    K = KITTI_K
    rng = np.random.default_rng(100 + n)
    for _ in range(2):
        R, t, X, X2 = _motion_case(rng, K, n=n)
        F = _fundamental(K, R, t)
        p1, p2 = _project(K, X).astype(np.float32), _project(K, X2).astype(np.float32)
        rc, Rr, tr, cnt = _assert_pose(ctx_stage, F, K, p1, p2, 1.0, n)
        assert rc == 0 and cnt.max() == n
        assert max(np.abs(Rr - R).max(), np.abs(tr - t).max()) <= 1e-9


def test_pose_other_intrinsics():
    """fx != fy and another principal point."""
    K = np.array([[700.0, 0.0, 300.0], [0.0, 650.0, 100.0], [0.0, 0.0, 1.0]])
    ctx = Context(W, H, K=K, max_kpts=N)
    try:
        winners = set()
        for i, (kind, F, p1, p2, Rt, tt) in enumerate(pose_battery(K, ncases=24, seed=13)):
            rc, R, t, cnt = _assert_pose(ctx, F, K, p1, p2, 1.0, (i, kind))
            assert rc == 0
            winners.add(int(np.argmax(cnt)))
            if kind in ("front", "swap"):
                assert max(np.abs(R - Rt).max(), np.abs(t - tt).max()) <= 1e-9
        assert len(winners) >= 2
        assert ctx.device_errors() == 0
    finally:
        ctx.close()


def test_pose_sparse_essential_matrices():
    """getPose's countNonZero(E) < 5 gate.  With a diagonal K (no principal point offset) K^T F K
    scales each entry of F on its own, so E's zeros are exact: axis-aligned translations with axis
    rotations give 2, 3 or 4 nonzero entries (VO_ERR_DEGENERATE_E), one more entry passes the gate."""
    K = np.diag([500.0, 400.0, 1.0])
    Ki = np.linalg.inv(K)
    c, s = math.cos(0.3), math.sin(0.3)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    ez, ex = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])
    E4 = _skew(ez) @ Rz
    E5 = E4.copy()
    E5[2, 2] = 0.5
    E5b = _skew(np.array([0.6, 0.0, 0.8]))
    E5b[0, 0] = 1e-3
    mats = [("tz", _skew(ez), 2), ("tz_Ry", _skew(ez) @ Ry, 3), ("tx_Rz", _skew(ex) @ Rz, 3), ("tz_Rz", E4, 4),
            ("txz", _skew(np.array([0.6, 0.0, 0.8])), 4), ("five", E5, 5), ("five_b", E5b, 5),
            ("six", _skew(np.array([0.6, 0.48, 0.64])), 6)]
    rng = np.random.default_rng(21)
    _, _, X, X2 = _motion_case(rng, K)
    p1, p2 = _project(K, X).astype(np.float32), _project(K, X2).astype(np.float32)
    ctx = Context(W, H, K=K, max_kpts=N)
    try:
        for name, E, nz in mats:
            assert np.count_nonzero(E) == nz, name
            F = Ki.T @ E @ Ki
            assert np.count_nonzero(K.T @ F @ K) == nz, name
            rc = _assert_pose(ctx, F, K, p1, p2, 1.0, name)[0]
            assert (rc != 0) == (nz < 5), (name, rc)
        assert ctx.device_errors() == 0
    finally:
        ctx.close()
