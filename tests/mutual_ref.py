"""Reference restatement of mutual-nearest-neighbour (cross-check) matching, built from the CPU
oracle's own stages (tests/test_mutual_reference.py validates it, tests/test_gpu_mutual_match.py
holds the GPU paths to it).

  forward   oracle.match: fwd[i] = the first-index minimum of (dist << 16 | j) over cur, accepted by
            a strict best < ratio * second on the top-2 distances;
  backward  back[j] = argmin_i (dist(i, j) << 16 | i) over prev: same distance (tests 0..31, or all
            512 at match_bits = 512), first-index minimum, no ratio test;
  mutual    (i, j) is kept iff fwd[i] == j and back[j] == i, in ascending i.

loop() restates the oracle's trajectory loop (voo_vo_process) from the oracle's stage wrappers, so a
filter can sit between the matcher and RANSAC; with no filter it must equal oracle.VO bit for bit.
"""
import numpy as np

import oracle as O

ST_OK, ST_FIRST, ST_MISSING, ST_FEW_MATCHES, ST_FEW_INLIERS, ST_DEGENERATE = 0, 1, 2, 3, 4, 5


def _test_bits(d, bits):
    """n x bits array of the descriptor tests in {0, 1} (32: the low half of word 0)."""
    d = np.ascontiguousarray(d, dtype=np.uint64).reshape(-1, 8)
    if bits == 32:
        w = np.ascontiguousarray((d[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        return np.unpackbits(w.view(np.uint8).reshape(-1, 4), axis=1)
    return np.unpackbits(d.view(np.uint8).reshape(-1, 64), axis=1)


def distances(d1, d2, bits):
    """n1 x n2 Hamming distances (int64).  |a ^ b| = |a| + |b| - 2 a.b; the f32 product is exact
    (integers up to 512)."""
    b1 = _test_bits(d1, bits).astype(np.float32)
    b2 = _test_bits(d2, bits).astype(np.float32)
    dot = (b1 @ b2.T).astype(np.int64)
    return b1.sum(1).astype(np.int64)[:, None] + b2.sum(1).astype(np.int64)[None, :] - 2 * dot


def back_best(d1, d2, bits):
    """back[j] for every cur keypoint j (n1 >= 1)."""
    D = distances(d1, d2, bits)
    key = (D << 16) | np.arange(D.shape[0], dtype=np.int64)[:, None]
    return np.argmin(key, axis=0).astype(np.int32)


def forward_pairs(d1, d2, bits, ratio):
    """The forward side in numpy with the same distance and key code as back_best: top-2 keys
    (dist << 16 | j) per prev keypoint, strict f32 ratio test.  Must reproduce oracle.match."""
    n1, n2 = np.asarray(d1).reshape(-1, 8).shape[0], np.asarray(d2).reshape(-1, 8).shape[0]
    if n1 == 0 or n2 < 2:
        return np.zeros((0, 2), np.int32)
    D = distances(d1, d2, bits)
    key = np.sort((D << 16) | np.arange(n2, dtype=np.int64)[None, :], axis=1)[:, :2]
    best, second = (key[:, 0] >> 16).astype(np.float32), (key[:, 1] >> 16).astype(np.float32)
    ok = best < np.float32(ratio) * second
    i = np.flatnonzero(ok)
    return np.stack([i, key[i, 0] & 0xFFFF], axis=1).astype(np.int32)


def mutual_filter(bits):
    def filt(d1, d2, pairs):
        if pairs.shape[0] == 0:
            return pairs
        back = back_best(d1, d2, bits)
        return pairs[back[pairs[:, 1]] == pairs[:, 0]]
    return filt


def mutual_pairs(d1, d2, bits, ratio):
    """oracle.match filtered by back[]."""
    d1 = np.ascontiguousarray(d1, dtype=np.uint64).reshape(-1, 8)
    d2 = np.ascontiguousarray(d2, dtype=np.uint64).reshape(-1, 8)
    if d1.shape[0] == 0 or d2.shape[0] == 0:
        return np.zeros((0, 2), np.int32)
    return mutual_filter(bits)(d1, d2, O.match(d1, d2, match_bits=bits, ratio=ratio))


def match_sets():
    """tests/test_gpu_stage_edges.py's crafted sets, {name: (queries, candidates)}: every crafted
    difference sits in tests 0..31, so both matcher widths see it."""
    rng = np.random.default_rng(3)
    d = rng.integers(0, 2**63, size=(64, 8), dtype=np.uint64)
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
    qs = rng.integers(0, 2**63, size=(70, 8), dtype=np.uint64)
    cs = qs[np.arange(257) % 70].copy()
    for j in range(257):
        for b in rng.choice(32, size=1 + (7 * j) % 5 + j // 70, replace=False):
            cs[j, 0] ^= np.uint64(1 << int(b))
    for nc in (2, 3, 64, 65, 257):
        sets["cands%d" % nc] = (qs, cs[:nc])
    return sets


_CASES = {}


def sequence_case(step, bits):
    """The 12-frame 320 x 192 scene sequence at `step` m/frame, max_kpts = 500: (frames, oracle
    config, plain loop rows, mutual loop rows, [(matches, kept)] per matched frame of the mutual
    loop).  Computed once per session and shared; callers must not modify it."""
    from acs_visual_odometry_amd.synth import SceneSequence
    key = (step, bits)
    if key not in _CASES:
        seq = SceneSequence(320, 192, nframes=12, step=step)
        frames = seq.frames()
        cfg = O.config(320, 192, K=seq.K.reshape(9), max_kpts=500, match_bits=bits)
        counts = []
        plain = loop(frames, cfg)
        mutual = loop(frames, cfg, mutual_filter(bits), counts)
        _CASES[key] = (frames, cfg, plain, mutual, counts)
    return _CASES[key]


def _mm4(A, B):
    """voo's mm4: ((a0 b0 + a1 b1) + a2 b2) + a3 b3 per entry, in Python floats (IEEE f64, no fma)."""
    return [((A[i * 4 + 0] * B[0 * 4 + j] + A[i * 4 + 1] * B[1 * 4 + j]) + A[i * 4 + 2] * B[2 * 4 + j]) +
            A[i * 4 + 3] * B[3 * 4 + j] for i in range(4) for j in range(4)]


def _push(T, flip):
    return np.array([(-T[r * 4 + c] if flip and r == 2 else T[r * 4 + c]) for r in range(3) for c in range(4)],
                    np.float64).reshape(3, 4)


def loop(frames, cfg, filt=None, counts=None):
    """voo_vo_process over `frames` (None = a missing image) without ground truth (scale 1), from
    oracle.extract / match / ransac (seeded voo_frame_seed) / pose.  filt(d_prev, d_cur, pairs) may
    drop matches before everything downstream.  Returns [(pose 3x4, status, info[8])]; counts, if a
    list, receives (matches before the filter, after) per matched frame."""
    L = O.lib()
    K = np.array(cfg.K[:], np.float64)
    T = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    prev = None                                   # desc1: (keypoints, descriptors) of the last valid frame
    model_F, model_p1, model_p2, model_n = None, None, None, 0
    rows = []
    for fi, g in enumerate(frames):
        info = np.zeros(8, np.int32)
        info[3] = -1
        if fi == 0:
            if g is not None:
                kp, de, _ = O.extract(g, cfg)
                prev = (kp, de)
            info[0] = 0 if prev is None else len(prev[0])
            rows.append((_push(T, 0), ST_FIRST, info))
            continue
        if g is None:
            rows.append((_push(T, 0), ST_MISSING, info))
            continue
        kc, dc, _ = O.extract(g, cfg)
        n_prev = 0 if prev is None else len(prev[0])
        pairs = O.match(prev[1], dc, match_bits=cfg.match_bits, ratio=cfg.ratio) if n_prev else np.zeros((0, 2), np.int32)
        m0 = pairs.shape[0]
        if filt is not None:
            pairs = filt(prev[1], dc, pairs)
        m = pairs.shape[0]
        if counts is not None:
            counts.append((m0, m))
        info[0], info[1] = len(kc), m
        if m < 8:
            rows.append((_push(T, 1), ST_FEW_MATCHES, info))
            continue
        pts = np.concatenate([prev[0][pairs[:, 0]], kc[pairs[:, 1]]], axis=1).astype(np.float64)
        rr = O.ransac(pts, prob=cfg.ransac_p, thr=cfg.sampson_thr, T=cfg.ransac_chunk_threads,
                      seed=L.voo_frame_seed(cfg.seed, fi), rng_mode=cfg.rng_mode)
        info[2], info[3], info[4], info[5] = rr["n_inl"], rr["best_k"], rr["n_evaluated"], rr["fitted"]
        if rr["fitted"]:                          # else the previous model leaks (quirk 9)
            model_F, model_n = rr["F"].copy(), rr["n_inl"]
            p = pts[rr["inliers"]].astype(np.float32)
            model_p1, model_p2 = p[:, :2].copy(), p[:, 2:].copy()
        if model_n < 8:
            rows.append((_push(T, 1), ST_FEW_INLIERS, info))
            continue
        prev = (kc, dc)                           # desc1 advances
        rc, R, t, _ = O.pose(model_F, K, model_p1, model_p2, 1.0)
        if rc != 0:
            rows.append((_push(T, 1), ST_DEGENERATE, info))
            continue
        R, t = [float(x) for x in R.reshape(9)], [float(x) for x in t]
        Trel = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0.0, 0.0, 0.0, 1.0]
        T = _mm4(T, Trel)
        rows.append((_push(T, 1), ST_OK, info))
    return rows
