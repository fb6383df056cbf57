"""Mutual-nearest-neighbour matching (vo_set_match_mode VO_MATCH_MUTUAL) on the GPU against the
reference restatement (tests/mutual_ref.py, validated on the CPU by tests/test_mutual_reference.py):
the stage call pair for pair, and every trajectory path row for row, bit for bit -- the per-frame
call, the device-resident and host-streamed batched calls, two sequences in one stream, two shards
of one sequence -- plus the mode's handling and the C++ facade's set_cross_check."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import mutual_ref as MR
import oracle as O
from acs_visual_odometry_amd import Context, VisualOdometry, _lib, shard
from acs_visual_odometry_amd.synth import SceneSequence

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "acs_visual_odometry_amd", "bin", "vo_cross_check_test")
W, H, N = 320, 192, 500
MUTUAL, RATIO = _lib.VO_MATCH_MUTUAL, _lib.VO_MATCH_RATIO
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 500]       # the 64-query and 256-query workgroup edges


def _flip(d, bits):
    """A copy of descriptor d (1 x 8) with the given tests (< 32, seen at both widths) flipped."""
    out = d.copy()
    for b in bits:
        out[0, 0] ^= np.uint64(1 << b)
    return out


def _mutual_sets():
    """{name: (prev, cur)} for the cross-check itself.  c is a candidate, far another one at distance
    16 from it (tests 16..31), so a query within a few tests of c passes the ratio test."""
    rng = np.random.default_rng(17)
    c = rng.integers(0, 2**63, size=(1, 8), dtype=np.uint64)
    far = _flip(c, range(16, 32))
    cur = np.concatenate([c, far])
    sets = {}
    # two queries whose best is c, at distances 3 and 1: only the nearer one keeps it
    sets["shared_nearer_second"] = (np.concatenate([_flip(c, [0, 1, 2]), _flip(c, [3])]), cur)
    sets["shared_nearer_first"] = (np.concatenate([_flip(c, [3]), _flip(c, [0, 1, 2])]), cur)
    # ... at equal distances: the lower prev index keeps it
    sets["shared_equal"] = (np.concatenate([_flip(c, [0]), _flip(c, [1]), _flip(c, [2])]), cur)
    # c0's nearest query q0 is at distance 1 from c0 and from c1, so the ratio test (0.75) rejects it;
    # q1 (3 from c0, 5 from c1) is accepted with c0, whose back[] is q0: c0 is given to nobody
    c1 = _flip(c, [8, 9])
    sets["back_is_rejected_query"] = (np.concatenate([_flip(c, [8]), _flip(c, [0, 1, 2])]), np.concatenate([c, c1]))
    d = rng.integers(0, 2**63, size=(40, 8), dtype=np.uint64)
    sets["one_by_n"] = (_flip(d[7:8], [4]), d)
    sets["n_by_one"] = (d, _flip(d[7:8], [4]))            # one candidate: no second best, no match
    sets["one_by_one"] = (d[:1], d[:1])
    return sets


def _planted(rng, n1, n2):
    """n1 x n2 random descriptors; about half of the smaller side planted as near-duplicates
    (1 .. 3 tests of the first 32 flipped), a quarter of those planted twice, so candidates are
    contested at different and at equal distances."""
    prev = rng.integers(0, 2**63, size=(n1, 8), dtype=np.uint64)
    cur = rng.integers(0, 2**63, size=(n2, 8), dtype=np.uint64)
    k = (min(n1, n2) + 1) // 2
    pi, cj = rng.permutation(n1)[:k], rng.permutation(n2)[:k]
    for a in range(k):
        j = cj[a - 1] if a % 4 == 3 else cj[a]            # every fourth: the previous one's candidate again
        prev[pi[a]] = cur[j]
        for b in rng.choice(32, size=1 + a % 3, replace=False):
            prev[pi[a], 0] ^= np.uint64(1 << int(b))
    return prev, cur


def _same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref), what


@pytest.mark.parametrize("ratio", [0.75, 1.5])
@pytest.mark.parametrize("bits", [32, 512])
def test_match_stage_crafted_sets(bits, ratio):
    sets = dict(MR.match_sets(), **_mutual_sets())
    ref = {k: MR.mutual_pairs(a, b, bits, ratio) for k, (a, b) in sets.items()}
    plain = {k: O.match(a, b, match_bits=bits, ratio=ratio) for k, (a, b) in sets.items()}
    # the regimes, on the reference
    assert ref["shared_nearer_second"].tolist() == [[1, 0]] and ref["shared_nearer_first"].tolist() == [[0, 0]]
    assert plain["shared_nearer_second"].tolist() == [[0, 0], [1, 0]]
    assert ref["shared_equal"].tolist() == [[0, 0]] and plain["shared_equal"].shape[0] == 3
    if ratio == 0.75:
        assert plain["back_is_rejected_query"].tolist() == [[1, 0]] and ref["back_is_rejected_query"].shape[0] == 0
    assert ref["one_by_n"].tolist() == [[0, 7]] and ref["n_by_one"].shape[0] == 0
    assert sum(r.shape[0] for r in ref.values()) < sum(p.shape[0] for p in plain.values())
    with Context(W, H, max_kpts=N, match_bits=bits, ratio=ratio, match_mode=MUTUAL) as ctx:
        assert ctx.match_mode() == MUTUAL
        for k, (a, b) in sets.items():
            _same(ctx.match(a, b), ref[k], k)
        a = sets["ties0"][0]
        assert ctx.match(a[:0], a).shape[0] == 0 and ctx.match(a, a[:0]).shape[0] == 0
        # the default mode on the same context: the oracle's matcher
        ctx.set_match_mode(RATIO)
        for k, (a, b) in sets.items():
            _same(ctx.match(a, b), plain[k], k)


@pytest.mark.parametrize("bits", [32, 512])
def test_match_stage_workgroup_edges(bits):
    """Random descriptors with planted, partly contested near-duplicates at every (n_prev, n_cur) of
    SIZES x SIZES: counts below, at and above a workgroup's queries on either side."""
    rng = np.random.default_rng(23)
    kept = dropped = 0
    with Context(W, H, max_kpts=N, match_bits=bits, match_mode=MUTUAL) as ctx:
        for n1 in SIZES:
            for n2 in SIZES:
                a, b = _planted(rng, n1, n2)
                ref = MR.mutual_pairs(a, b, bits, 0.75)
                _same(ctx.match(a, b), ref, (n1, n2))
                kept += ref.shape[0]
                dropped += O.match(a, b, match_bits=bits, ratio=0.75).shape[0] - ref.shape[0]
        assert kept > 1000 and dropped > 100, (kept, dropped)
        ctx.set_match_mode(RATIO)
        a, b = _planted(rng, 257, 500)
        _same(ctx.match(a, b), O.match(a, b, match_bits=bits, ratio=0.75), "ratio mode")


def test_match_stage_512_across_the_lds_tile():
    """1025 keypoints on each side at 512 tests: both directions stream a second LDS tile."""
    rng = np.random.default_rng(29)
    a, b = _planted(rng, 1025, 1025)
    a[1024] = b[1024]                                     # a pair that lives in the second tile on both sides
    ref = MR.mutual_pairs(a, b, 512, 0.75)
    plain = O.match(a, b, match_bits=512, ratio=0.75)
    assert [1024, 1024] in ref.tolist() and 300 < ref.shape[0] < plain.shape[0]
    with Context(W, H, max_kpts=1100, match_bits=512, match_mode=MUTUAL) as ctx:
        _same(ctx.match(a, b), ref, "mutual")
        ctx.set_match_mode(RATIO)
        _same(ctx.match(a, b), plain, "ratio")


# ---------------------------------------------------------------------------------------------
# trajectory paths
# ---------------------------------------------------------------------------------------------

def _check(ref, poses, st, info):
    assert len(ref) == len(st)
    for f, (pr, sr, ir) in enumerate(ref):
        assert st[f] == sr, (f, st[f], sr)
        assert np.array_equal(info[f, :6], ir[:6]), (f, info[f], ir)
        assert np.array_equal(poses[f], pr), f


def _ctx(cfg, **kw):
    return Context(W, H, K=np.array(cfg.K[:]), max_kpts=cfg.max_kpts, match_bits=cfg.match_bits, **kw)


def _run(ctx, frames, path):
    if path == "frame":
        out = [ctx.process_frame(fr) for fr in frames]
        return (np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.stack([o[2] for o in out]))
    if path == "host":
        return ctx.process_frames_host(frames)
    df = ctx.device_frames(frames)
    try:
        return ctx.process_frames_device(df)
    finally:
        df.free()


@pytest.mark.parametrize("path,batch", [("frame", 0), ("device", 0), ("device", 4), ("host", 0)])
@pytest.mark.parametrize("step,bits", [(0.12, 32), (1.0, 32), (0.12, 512)])
def test_trajectory_paths_equal_the_mutual_loop(step, bits, path, batch):
    """12 frames through the per-frame call, the device-resident batched call (default batch and
    windows of 4 frames) and host streaming.  The 1.0 m/frame sequence starts with frames without a
    model and later poses from leaked models: the batched paths' speculation misses, repair windows
    and dual match records."""
    frames, cfg, plain, mutual, _ = MR.sequence_case(step, bits)
    with _ctx(cfg, match_mode=MUTUAL, frame_batch=batch) as ctx:
        out = _run(ctx, frames, path)
        assert ctx.device_errors() == 0
    _check(mutual, *out)


def test_two_sequences_in_one_stream():
    """2 x 6 frames (0.12 and 1.0 m/frame) as one stream: each sequence equals its own mutual loop."""
    parts = [MR.sequence_case(0.12, 32), MR.sequence_case(1.0, 32)]
    cfg = parts[0][1]
    frames = np.concatenate([p[0][:6] for p in parts])
    # a loop's first six rows depend on its first six frames only
    refs = [p[3][:6] for p in parts]
    with _ctx(cfg, match_mode=MUTUAL) as ctx:
        ctx.set_sequence_starts([6])
        poses, st, info = _run(ctx, frames, "device")
        assert ctx.device_errors() == 0
    assert st[0] == 1 and st[6] == 1
    for s in range(2):
        sl = slice(6 * s, 6 * s + 6)
        _check(refs[s], poses[sl], st[sl], info[sl])


def test_two_shards_of_one_sequence():
    """shard.run_local over two contexts built with match_mode: the keyword reaches every shard
    (ContextEngine.run resets its context, which keeps the mode)."""
    frames, cfg, _, mutual, _ = MR.sequence_case(0.12, 32)
    ctxs = [_ctx(cfg, match_mode=MUTUAL) for _ in range(2)]
    try:
        res = shard.run_local([shard.ContextEngine(c, frames) for c in ctxs], len(frames))
        assert all(c.match_mode() == MUTUAL and c.device_errors() == 0 for c in ctxs)
    finally:
        for c in ctxs:
            c.close()
    poses = np.concatenate([r.poses for r in res])
    st = np.concatenate([r.status for r in res])
    info = np.concatenate([r.info for r in res])
    _check(mutual, poses, st, info)


def test_mode_handling():
    frames, cfg, plain, mutual, _ = MR.sequence_case(0.12, 32)
    L = _lib.load()
    with _ctx(cfg) as fresh:
        assert fresh.match_mode() == RATIO
        assert fresh.kernel_forms()["match"] == ["k_match"]
        base = _run(fresh, frames, "device")
    _check(plain, *base)
    with _ctx(cfg) as ctx:
        ctx.set_match_mode(MUTUAL)
        assert ctx.kernel_forms()["match"] == ["k_match_mutual"]
        _check(mutual, *_run(ctx, frames, "device"))
        # an invalid mode is refused and changes nothing
        for bad in (2, -1, 1 << 20):
            assert L.vo_set_match_mode(ctx.h, bad) == -1
            with pytest.raises(RuntimeError):
                ctx.set_match_mode(bad)
        assert ctx.match_mode() == MUTUAL
        # the mode survives reset()
        ctx.reset()
        assert ctx.match_mode() == MUTUAL
        _check(mutual, *_run(ctx, frames, "frame"))
        # back to the ratio mode: a fresh default context's rows
        ctx.reset()
        ctx.set_match_mode(RATIO)
        assert ctx.kernel_forms()["match"] == ["k_match"]
        out = _run(ctx, frames, "device")
        assert all(np.array_equal(a, b) for a, b in zip(out, base))
    with _ctx(MR.sequence_case(0.12, 512)[1], match_mode=MUTUAL) as c512:
        assert c512.kernel_forms()["match"] == ["k_match_mutual"]        # one template for both widths
        c512.set_match_mode(RATIO)
        assert c512.kernel_forms()["match"] == ["k_match512"]
    with pytest.raises(RuntimeError):
        _ctx(cfg, match_mode=7)


def test_python_facade_cross_check():
    frames, cfg, _, _, _ = MR.sequence_case(0.12, 32)
    vo = VisualOdometry(width=W, height=H, max_kpts=N, cross_check=True)
    try:
        assert vo.ctx.match_mode() == MUTUAL
        (d1, _), (d2, _) = (vo.compute_descriptor_with_key_points(frames[f]) for f in (0, 1))
        got = vo.match_descriptors(d1, d2)
    finally:
        vo.ctx.close()
    e = [O.extract(frames[f], cfg) for f in (0, 1)]
    assert got == [tuple(map(int, r)) for r in MR.mutual_pairs(e[0][1], e[1][1], 32, 0.75)]
    plain = VisualOdometry(width=W, height=H, max_kpts=N)
    try:
        assert plain.ctx.match_mode() == RATIO
    finally:
        plain.ctx.close()


def test_cpp_facade_set_cross_check(tmp_path):
    """include/VisualOdometry.hpp set_cross_check through a g++ binary (tests/cpp/cross_check_test.cpp):
    one frame pair's mutual match count and pairs equal the restatement's."""
    assert os.access(BIN, os.X_OK), "make -C acs_visual_odometry_amd/csrc builds it"
    seq = SceneSequence(nframes=2, step=0.12)
    paths = []
    for f in range(2):
        paths.append(str(tmp_path / f"{f:06d}.pgm"))
        Image.fromarray(seq.frame(f)).save(paths[-1])
    cfg = O.config(seq.W, seq.H)
    e = [O.extract(seq.frame(f), cfg) for f in range(2)]
    ref = MR.mutual_pairs(e[0][1], e[1][1], 32, 0.75)
    plain = O.match(e[0][1], e[1][1])
    assert 8 <= ref.shape[0] < plain.shape[0]
    r = subprocess.run([BIN, paths[0], paths[1], str(ref.shape[0])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[:200], r.stderr)
    lines = dict((ln.split()[0], ln.split()[1:]) for ln in r.stdout.splitlines())
    assert lines["plain"] == [str(plain.shape[0]), "mutual", str(ref.shape[0]), "again", str(plain.shape[0])]
    assert np.array_equal(np.array(lines["pairs"], np.int32).reshape(-1, 2), ref)
    # a wrong expectation fails the binary: its check is live
    r = subprocess.run([BIN, paths[0], paths[1], str(ref.shape[0] + 1)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1
