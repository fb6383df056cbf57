"""GPU parity away from the reference defaults: resp_thr, the NMS borders, ratio, and the whole
path with every tunable field changed, against the CPU oracle with the same config, bit for bit.

The other GPU tests all create their contexts with resp_thr 20000, borders 35 / 37, ratio 0.75,
ransac_p 0.99 and sampson_thr 1.0.  Here each case first asserts on the oracle's own output that
it is the regime it claims (a full top bin, a strict-compare boundary, two survivors, none, fewer
than N inside the borders, ...), then compares the HIP path.  Frames are 320 x 192 with N = 500,
where the stencil has 6 x 12 tiles and the select still ranks more candidates than N.
"""
import numpy as np
import pytest

import oracle as O
from acs_visual_odometry_amd import Context
from acs_visual_odometry_amd.synth import SceneSequence, noise_frames

pytestmark = pytest.mark.gpu
W, H, N = 320, 192, 500
MIN_BORDER = 35          # vo_create's minimum for both borders (tests/test_abi.py derives it)


@pytest.fixture(scope="module")
def scene():
    seq = SceneSequence(W, H, nframes=8, step=0.05)
    return seq, seq.frames()


@pytest.fixture(scope="module")
def images(scene):
    return {"scene": scene[1][0], "noise": noise_frames(W, H, 1)[0]}


def _maxima(img, brow=35, bcol=37):
    """Responses of every NMS maximum inside the borders, descending (no threshold, no top-N)."""
    R0 = O.response(O.blur7(img), 0.0)
    k = O.nms_topn(R0, N=W * H, brow=brow, bcol=bcol)
    return np.sort(R0[k[:, 1], k[:, 0]])[::-1]


def _threshold(name, img):
    """The resp_thr of a named case and the keypoint count it must leave on the oracle."""
    v = _maxima(img)
    assert v.size > N and v[N - 2] > v[N - 1] > v[N]          # more candidates than N, no tie at the cut
    f = np.float32
    if name == "zero":
        return f(0.0), N
    if name == "one":
        return f(1.0), N
    if name == "nth":                              # strict compare: the N-th keypoint itself drops out
        return v[N - 1], N - 1
    if name == "nth_up":
        return np.nextafter(v[N - 1], f(np.inf)), N - 1
    if name == "nth_down":
        return np.nextafter(v[N - 1], f(0.0)), N
    if name == "two":
        assert v[1] > v[2]
        thr = f(0.5) * (v[1] + v[2])
        assert v[1] > thr >= v[2]
        return thr, 2
    assert name == "none"
    assert v[0] < 1e7
    return f(1e7), 0


def _check_extract(monkeypatch, sel1, kind, images, thr, brow, bcol, expect_n):
    """vo_extract, vo_response and vo_extract_frames_device (3 frames: the banded select of small
    batches; 24 frames: the one-workgroup select with its own LDS histogram) against the oracle."""
    if sel1:
        monkeypatch.setenv("VO_SEL1", sel1)
    img, other = images[kind], images["noise" if kind == "scene" else "scene"]
    cfg = O.config(W, H, max_kpts=N, resp_thr=float(thr), border_row=brow, border_col=bcol)
    ref = {"img": O.extract(img, cfg)[:2], "other": O.extract(other, cfg)[:2]}
    # the regime, on the oracle
    Rr = O.response(O.blur7(img), float(thr))
    cand = O.nms_candidates(Rr, brow=brow, bcol=bcol)
    n_ref = ref["img"][0].shape[0]
    assert n_ref == min(cand, N)
    if callable(expect_n):
        assert expect_n(cand), cand
    else:
        assert n_ref == expect_n and (expect_n < N or cand >= N), (n_ref, cand)
    if float(thr) == 0.0 and brow == 35 and bcol == 37:
        assert cand > N                            # the whole ranking happens inside the clamped top bin
    ctx = Context(W, H, max_kpts=N, resp_thr=float(thr), border_row=brow, border_col=bcol)
    try:
        k, d = ctx.extract(img)
        assert k.shape == ref["img"][0].shape, (k.shape, ref["img"][0].shape)
        assert np.array_equal(k, ref["img"][0]), "keypoints differ"
        assert np.array_equal(d, ref["img"][1]), "descriptor bits differ"
        R = ctx.response(img)
        assert np.array_equal(R.view(np.uint32), Rr.view(np.uint32)), "response map differs"
        for nb in (3, 24):
            order = ["img", "other"] * (nb // 2) + ["img"] * (nb % 2)
            df = ctx.device_frames(np.stack([img if o == "img" else other for o in order]))
            nk, kl, dl = ctx.extract_frames_device(df, outputs=True)
            df.free()
            for f, o in enumerate(order):
                assert nk[f] == ref[o][0].shape[0], (nb, f, nk[f])
                assert np.array_equal(kl[f], ref[o][0]), (nb, f)
                assert np.array_equal(dl[f], ref[o][1]), (nb, f)
        assert ctx.device_errors() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("sel1", ["", "0", "1"])
@pytest.mark.parametrize("name", ["zero", "one", "nth", "nth_up", "nth_down", "two", "none"])
@pytest.mark.parametrize("kind", ["scene", "noise"])
def test_extract_thresholds_bit_exact(kind, name, sel1, images, monkeypatch):
    """resp_thr from 0 (every key in the select's clamped top bin: the boundary-list radix select
    ranks everything) over the N-th keypoint's own response and its two f32 neighbours (the strict
    compare decides whether N or N - 1 keypoints come out) up to thresholds that leave 2 and 0."""
    thr, n = _threshold(name, images[kind])
    _check_extract(monkeypatch, sel1, kind, images, thr, 35, 37, n)


# (border_row, border_col): the minimum vo_create accepts, and two asymmetric pairs
BORDERS = [(MIN_BORDER, MIN_BORDER), (60, 90), (41, 77)]


@pytest.mark.parametrize("sel1", ["", "0", "1"])
@pytest.mark.parametrize("thr", [0.0, 150000.0])
@pytest.mark.parametrize("brow,bcol", BORDERS)
@pytest.mark.parametrize("kind", ["scene", "noise"])
def test_extract_borders_bit_exact(kind, brow, bcol, thr, sel1, images, monkeypatch):
    """The stencil's NMS masks and the describe at other borders: at the minimum the rotated samples
    touch the frame's first and last rows and columns; (60, 90) leaves fewer than N candidates even
    at threshold 0; at 150000 few survive anywhere."""
    v = _maxima(images[kind], brow, bcol)
    want = int((v > np.float32(thr)).sum())
    if thr == 0.0:
        full = {(MIN_BORDER, MIN_BORDER): True, (60, 90): False, (41, 77): kind == "noise"}[(brow, bcol)]
        assert (want > N) == full and want > 0, want
    else:
        assert 0 < want < N, want
    _check_extract(monkeypatch, sel1, kind, images, np.float32(thr), brow, bcol, lambda cand: cand == want)


def test_minimum_borders_reach_the_frame_edges(images):
    """Premise of the minimum-border cases: on the oracle, keypoints sit on the border lines, so the
    describe's rotated samples (offsets -35 .. +34) start at row / column 0 and end at the last."""
    cfg = O.config(W, H, max_kpts=N, resp_thr=0.0, border_row=MIN_BORDER, border_col=MIN_BORDER)
    xs, ys = [], []
    for img in images.values():
        k = O.extract(img, cfg)[0]
        xs += list(k[:, 0])
        ys += list(k[:, 1])
    assert min(xs) == MIN_BORDER and max(xs) == W - MIN_BORDER
    assert min(ys) == MIN_BORDER and max(ys) == H - MIN_BORDER


@pytest.mark.parametrize("sel1", ["", "1"])
def test_kitti_batch_full_top_bin(sel1, monkeypatch):
    """1241 x 376, N = 2000, resp_thr = 0 through the batched extract of 24 frames: the KITTI path's
    one-workgroup select builds its histogram in LDS, and every key is in the clamped top bin."""
    if sel1:
        monkeypatch.setenv("VO_SEL1", sel1)
    seq = SceneSequence(nframes=2, step=0.05)
    frames = seq.frames()
    cfg = O.config(seq.W, seq.H, resp_thr=0.0)
    ref = [O.extract(f, cfg)[:2] for f in frames]
    for f in frames:
        assert O.nms_candidates(O.response(O.blur7(f), 0.0)) > 2000
    ctx = Context(seq.W, seq.H, resp_thr=0.0)
    df = ctx.device_frames(np.concatenate([frames] * 12))
    nk, kl, dl = ctx.extract_frames_device(df, outputs=True)
    df.free()
    for f in range(24):
        assert nk[f] == 2000
        assert np.array_equal(kl[f], ref[f % 2][0]), f
        assert np.array_equal(dl[f], ref[f % 2][1]), f
    k, d = ctx.extract(frames[1])
    assert np.array_equal(k, ref[1][0]) and np.array_equal(d, ref[1][1])
    assert ctx.device_errors() == 0
    ctx.close()


RATIOS = [("0", np.float32(0.0)), ("0.5", np.float32(0.5)),
          ("0.75-", np.nextafter(np.float32(0.75), np.float32(0.0))), ("0.75", np.float32(0.75)),
          ("0.75+", np.nextafter(np.float32(0.75), np.float32(1.0))), ("1", np.float32(1.0)),
          ("1.5", np.float32(1.5))]


@pytest.mark.parametrize("bits", [32, 512])
def test_match_ratios_bit_exact(bits, scene):
    """ratio_accept's f32 product at other ratios than 0.75, both matcher widths.  Premises on the
    oracle: the match count grows strictly over 0 / 0.5 / 0.75 / 1 / 1.5; 0 accepts nothing and 1.5
    every query; one ulp above 0.75 accepts the 3 : 4 distance pairs that 0.75 itself rejects,
    one ulp below changes nothing."""
    seq, frames = scene
    cfg = O.config(W, H, max_kpts=N)
    d0, d1 = O.extract(frames[0], cfg)[1], O.extract(frames[1], cfg)[1]
    assert d0.shape[0] == N and d1.shape[0] == N
    ref = {name: O.match(d0, d1, match_bits=bits, ratio=float(r)) for name, r in RATIOS}
    n = {name: m.shape[0] for name, m in ref.items()}
    assert 0 == n["0"] < n["0.5"] < n["0.75"] < n["1"] < n["1.5"] == N, n
    assert n["0.75-"] == n["0.75"] < n["0.75+"], n
    for name, r in RATIOS:
        ctx = Context(W, H, max_kpts=N, match_bits=bits, ratio=float(r))
        try:
            m = ctx.match(d0, d1)
            assert m.shape == ref[name].shape, (name, m.shape, ref[name].shape)
            assert np.array_equal(m, ref[name]), name
        finally:
            ctx.close()


OFF_DEFAULT = dict(resp_thr=5000.0, border_row=40, border_col=45, ratio=0.9, sampson_thr=0.25, ransac_p=0.999,
                   ransac_chunk_threads=3, max_kpts=N)


@pytest.fixture(scope="module")
def off_default_rows(scene):
    seq, frames = scene
    rows = {}
    for tag, kw in (("off", OFF_DEFAULT), ("default", dict(max_kpts=N))):
        vo = O.VO(O.config(W, H, K=seq.K.reshape(9), **kw), gt=seq.gt())
        rows[tag] = [vo.process(f) for f in frames]
        vo.close()
    ref, dflt = rows["off"], rows["default"]
    # the regime: every frame after the first is posed from a model fitted on that frame, and the
    # config reaches the result (counts and poses differ from the default config's on every frame)
    assert ref[0][1] == 1 and all(r[1] == 0 and r[2][5] == 1 for r in ref[1:]), [(r[1], list(r[2][:6])) for r in ref]
    for f in range(1, len(frames)):
        assert not np.array_equal(ref[f][2][:3], dflt[f][2][:3]), f
        assert not np.array_equal(ref[f][0], dflt[f][0]), f
    return ref


def _assert_rows(ref, poses, st, info):
    for f, (pr, sr, ir) in enumerate(ref):
        assert st[f] == sr, (f, st[f], sr)
        assert np.array_equal(info[f][:6], ir[:6]), (f, info[f], ir)
        assert np.array_equal(poses[f], pr), f


@pytest.mark.parametrize("route", ["process_frame", "process_frames_device", "process_frames_host"])
def test_whole_path_off_default(route, scene, off_default_rows):
    """Eight frames with resp_thr 5000, borders 40 / 45, ratio 0.9, sampson_thr 0.25, ransac_p 0.999 and
    T = 3: the per-frame call (fused wave-form RANSAC) and the batched routes (group form, batch 3)
    both count inliers by num / den < thr, and draw their bounds from 0.999's table."""
    seq, frames = scene
    ctx = Context(W, H, K=seq.K, frame_batch=3 if route == "process_frames_device" else 0, **OFF_DEFAULT)
    ctx.set_ground_truth(seq.gt())
    try:
        if route == "process_frame":
            out = [ctx.process_frame(f) for f in frames]
            poses, st, info = [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]
        elif route == "process_frames_device":
            df = ctx.device_frames(frames)
            poses, st, info = ctx.process_frames_device(df)
            df.free()
        else:
            poses, st, info = ctx.process_frames_host(frames)
        _assert_rows(off_default_rows, poses, st, info)
        assert ctx.device_errors() == 0
    finally:
        ctx.close()
