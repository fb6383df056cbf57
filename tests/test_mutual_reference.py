"""The reference restatement of mutual-nearest-neighbour matching (tests/mutual_ref.py) against the
CPU oracle, before tests/test_gpu_mutual_match.py trusts it with the filter; the regime the GPU
tests rely on, asserted on the reference alone; and the binding of vo_set_match_mode."""
import os
import re

import numpy as np
import pytest

import mutual_ref as MR
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ratio", [0.75, 1.5])
@pytest.mark.parametrize("bits", [32, 512])
def test_numpy_forward_side_reproduces_the_oracle_matcher(bits, ratio):
    """The distance and key code back[] uses, pointed the other way: top-2 keys (dist << 16 | j) and
    the strict ratio give oracle.match on the crafted sets (ties, equal best and second, zero
    distances, 2 .. 257 candidates)."""
    n_pairs = 0
    for name, (a, b) in MR.match_sets().items():
        ref = O.match(a, b, match_bits=bits, ratio=ratio)
        got = MR.forward_pairs(a, b, bits, ratio)
        assert got.shape == ref.shape and np.array_equal(got, ref), name
        n_pairs += ref.shape[0]
    assert n_pairs > 100


def test_distances_are_hamming_distances():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 2**63, size=(7, 8), dtype=np.uint64)
    b = rng.integers(0, 2**63, size=(9, 8), dtype=np.uint64)
    for bits in (32, 512):
        D = MR.distances(a, b, bits)
        for i in range(7):
            for j in range(9):
                if bits == 32:
                    ref = bin((int(a[i, 0]) ^ int(b[j, 0])) & 0xFFFFFFFF).count("1")
                else:
                    ref = sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a[i], b[j]))
                assert D[i, j] == ref


@pytest.mark.parametrize("step", [0.12, 1.0])
def test_loop_restatement_equals_the_oracle_loop(step):
    """loop(filter=None) is voo_vo_process without ground truth: status, info[:6] and pose rows,
    bit for bit, including the frames without a fit of their own at 1.0 m/frame."""
    frames, cfg, plain, _, _ = MR.sequence_case(step, 32)
    vo = O.VO(cfg)
    ref = [vo.process(frames[f]) for f in range(len(frames))]
    vo.close()
    assert len(plain) == len(ref) == 12
    for f, ((pg, sg, ig), (pr, sr, ir)) in enumerate(zip(plain, ref)):
        assert sg == sr, (f, sg, sr)
        assert np.array_equal(ig[:6], ir[:6]), (f, ig, ir)
        assert np.array_equal(pg, pr), (f, pg, pr)
    st = [r[1] for r in ref]
    assert st[0] == MR.ST_FIRST
    if step == 1.0:
        # no frame fits a model of its own here: every later frame leaves the loop at model_n < 8
        assert all(r[2][5] == 0 for r in ref[1:]) and set(st[1:]) == {MR.ST_FEW_INLIERS}
    else:
        assert set(st[1:]) == {MR.ST_OK}


@pytest.mark.parametrize("step", [0.12, 1.0])
def test_mutual_filter_bites_at_32_bits(step):
    """Regime, on the reference alone: at 32 tests the filter removes a match on every frame >= 1, the
    kept pairs are fewer, and the mutual loop's rows differ from the plain loop's (so a library without
    the mode cannot pass the GPU tests)."""
    _, _, plain, mutual, counts = MR.sequence_case(step, 32)
    assert len(counts) == 11
    assert all(kept < m0 for m0, kept in counts), counts
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(plain, mutual))
    if step == 1.0:
        # the batched paths' speculation misses: early frames without a model, and later frames
        # that pose with the previous frame's model (no fit of their own)
        st, fit = [r[1] for r in mutual], [int(r[2][5]) for r in mutual]
        assert st[1] == MR.ST_FEW_INLIERS and MR.ST_OK in st
        assert any(s == MR.ST_OK and not f for s, f in zip(st, fit))


def test_mutual_filter_at_512_bits():
    """At 512 tests a frame pair may lose nothing; over the sequence the filter removes matches."""
    _, _, _, _, counts = MR.sequence_case(0.12, 512)
    assert all(kept <= m0 for m0, kept in counts)
    assert sum(k for _, k in counts) < sum(m for m, _ in counts), counts


def test_mutual_pairs_is_a_subsequence_with_unique_candidates():
    rng = np.random.default_rng(11)
    a = rng.integers(0, 2**63, size=(120, 8), dtype=np.uint64)
    b = a[rng.permutation(120)[:90]].copy()
    b[:, 0] ^= np.uint64(1) << rng.integers(0, 32, size=90).astype(np.uint64)
    for bits in (32, 512):
        plain = O.match(a, b, match_bits=bits, ratio=0.75)
        mut = MR.mutual_pairs(a, b, bits, 0.75)
        assert 0 < mut.shape[0] <= plain.shape[0]
        assert set(map(tuple, mut)) <= set(map(tuple, plain))
        assert np.all(np.diff(mut[:, 0]) > 0)
        assert len(set(mut[:, 1])) == mut.shape[0]           # a candidate is given to one query only


def test_match_mode_is_declared_and_bound():
    """vo_set_match_mode / vo_match_mode and the two mode constants: in the header, in the binding's
    export list with argtypes, and in the library."""
    from acs_visual_odometry_amd import _lib
    src = open(os.path.join(ROOT, "include", "vo_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+vo_set_match_mode\s*\(\s*vo_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+vo_match_mode\s*\(\s*vo_ctx\s*\*\s*\w*\s*\)\s*;", code)
    assert re.search(r"#define\s+VO_MATCH_RATIO\s+0\b", code) and re.search(r"#define\s+VO_MATCH_MUTUAL\s+1\b", code)
    assert {"vo_set_match_mode", "vo_match_mode"} <= set(_lib.EXPORTS)
    assert (_lib.VO_MATCH_RATIO, _lib.VO_MATCH_MUTUAL) == (0, 1)
    L = _lib.load()
    assert L.vo_set_match_mode.argtypes is not None and L.vo_match_mode.argtypes is not None
    # host-only behaviour: a null context is an argument error
    assert L.vo_set_match_mode(None, 1) == -1 and L.vo_match_mode(None) == -1
