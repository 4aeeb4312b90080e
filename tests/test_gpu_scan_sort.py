"""The two device-wide primitives of csrc/scan_sort.hip -- exclusive_scan_u32 and radix_sort_pairs -- on their own, against numpy.

Every subsystem stands on them (tile-list offsets, densification surgery, mesh compaction; depth sort, knn Morton sort, the deterministic
backward's id sort), and the pipeline tests reach them only at the sizes their scenes happen to produce.  Here they are called through the
tests-only entry points ibgs_debug_scan_u32 / ibgs_debug_sort_pairs (api.hip; declared with ctypes below, not in include/) at the sizes where the
code changes path: the 2048-element scan chunk and its square (a third scan level), the 4096-key sort chunk, one to four passes of 6-, 7- and
8-bit digits, an odd pass count with its copy-back, both kinds of passes (ibgs_debug_set_onesweep) and the size at which the library itself
switches from one to the other.

Everything is integer: the reference is numpy, every comparison is array_equal.  Every buffer a primitive may write -- the output, both key and
both value buffers, the scratch at exactly the size *_scratch_elems returns -- ends in GUARD words of a sentinel that must survive the call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ibgs_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5C31E77
DROPPED = 0xFFFFFFFF          # the key radix_sort_pairs may leave out when it is given a kept_dev word (common.h)
BY_SIZE, CLASSIC, SINGLE_LAUNCH = -1, 0, 1


@functools.lru_cache(maxsize=None)
def lib():
    l = _lib.load()
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32
    l.ibgs_debug_scan_scratch_elems.restype = sz
    l.ibgs_debug_scan_scratch_elems.argtypes = [sz]
    l.ibgs_debug_scan_u32.restype = i32
    l.ibgs_debug_scan_u32.argtypes = [vp, vp, vp, sz, vp, sz, i32]
    l.ibgs_debug_sort_scratch_elems.restype = sz
    l.ibgs_debug_sort_scratch_elems.argtypes = [sz]
    l.ibgs_debug_sort_pairs.restype = i32
    l.ibgs_debug_sort_pairs.argtypes = [vp, vp, vp, vp, vp, sz, i32, vp, sz, vp, vp]
    l.ibgs_debug_set_onesweep.restype = i32
    l.ibgs_debug_set_onesweep.argtypes = [i32]
    return l


def dev(words, valid=None):
    """`words` (uint32) on the device, padded with the sentinel up to `valid` words, then GUARD words of the sentinel."""
    words = np.asarray(words, dtype=np.uint32)
    host = np.full((len(words) if valid is None else valid) + GUARD, SENTINEL, np.uint32)
    host[:len(words)] = words
    return torch.from_numpy(host.view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def untouched(words):
    return np.array_equal(words, np.full(len(words), SENTINEL, np.uint32))


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- scan --------------------------------------------------------------------------------------------------------------------------------
SQ = 2048 * 2048          # one element more needs a third scan level
SCAN_SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, SQ - 1, SQ, SQ + 1, SQ + 2049]
WRAP_SIZES = (65, 2049, 4097, SQ + 1)          # also scanned with full-range words: the running sum wraps 2^32 many times


def scan_reference(v):
    """(n + 1,) exclusive prefix sums mod 2^32; the last one is the total."""
    out = np.zeros(len(v) + 1, np.uint64)
    np.cumsum(v.astype(np.uint64), out=out[1:])
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def run_scan(v, in_place, with_total, scratch_short=0):
    n = len(v)
    elems = lib().ibgs_debug_scan_scratch_elems(n)
    src = dev(v, n + 1)
    out = src if in_place else dev([], n + 1)
    scratch = dev([], elems)
    rc = lib().ibgs_debug_scan_u32(stream(), src.data_ptr(), out.data_ptr(), n, scratch.data_ptr(), elems - scratch_short, 1 if with_total else 0)
    torch.cuda.synchronize()
    return rc, host(src), host(out), host(scratch), elems


def scan_inputs(n):
    rng = np.random.default_rng(1000 + n % 9973)
    yield "counts", rng.integers(0, 4, n, dtype=np.uint32)          # what the callers feed: tiles touched, keep masks, faces kept
    yield "ones", np.ones(n, np.uint32)
    if n in WRAP_SIZES:
        yield "wrapping", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_matches_cumsum(n):
    for name, v in scan_inputs(n):
        want = scan_reference(v)
        if name == "ones":
            assert np.array_equal(want[:n], np.arange(n, dtype=np.uint32))          # the expected output is the index
        for in_place in (False, True):
            for with_total in (False, True):
                what = "%s n=%d in_place=%s with_total=%s" % (name, n, in_place, with_total)
                rc, src, out, scratch, elems = run_scan(v, in_place, with_total)
                assert rc == 0, (what, _lib.last_error())
                assert np.array_equal(out[:n], want[:n]), what
                if with_total:
                    assert out[n] == want[n], what          # (n = 0: out[0] = 0)
                    assert untouched(out[n + 1:]), what
                else:
                    assert untouched(out[n:]), what          # out[n] included
                assert untouched(scratch[elems:]), what
                if not in_place:
                    assert np.array_equal(src[:n], v) and untouched(src[n:]), what


@pytest.mark.parametrize("n", [2049, SQ, SQ + 1, SQ + 2049])
def test_scan_refuses_a_scratch_one_element_short(n):
    """Host-side check, before any launch: a negative code, `out` as it was."""
    v = np.ones(n, np.uint32)
    for with_total in (False, True):
        rc, src, out, scratch, elems = run_scan(v, False, with_total, scratch_short=1)
        assert rc < 0
        assert "scratch" in _lib.last_error()
        assert untouched(out) and untouched(scratch)
        assert np.array_equal(src[:n], v)


# ---- sort --------------------------------------------------------------------------------------------------------------------------------
CHUNK = 4096
SORT_SIZES = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 8 * CHUNK + 1, 300001]          # 300001: 74 chunks, the look-back walks several batches of 8
# passes x digit bits: 1 -> 1 x 1, 7 -> 1 x 7, 8 -> 1 x 8, 13 -> 2 x 7, 17 -> 3 x 6, 20 -> 3 x 7, 24 -> 3 x 8, 30 and 32 -> 4 x 8
# (an odd pass count ends with the copy-back; 32, 30 and 20-ish bits are what the depth sort, the knn and the deterministic backward use)
WIDTHS = [1, 7, 8, 13, 17, 20, 24, 30, 32]
SHAPES = [(n, b) for b in (32, 20) for n in SORT_SIZES] + [(n, b) for b in WIDTHS if b not in (32, 20) for n in (CHUNK + 1, 300001)]
MODES = [CLASSIC, SINGLE_LAUNCH]


def stable_reference(keys, vals):
    """The one stable sort by key: a single sort of key << 32 | position."""
    packed = np.sort((keys.astype(np.uint64) << np.uint64(32)) | np.arange(len(keys), dtype=np.uint64))
    return (packed >> np.uint64(32)).astype(np.uint32), vals[(packed & np.uint64(0xFFFFFFFF)).astype(np.int64)]


def key_sets(n, nbits):
    """name -> n keys below 2^nbits"""
    rng = np.random.default_rng(n * 64 + nbits)
    top = (1 << nbits) - 1
    uniform = rng.integers(0, top + 1, n, dtype=np.uint64).astype(np.uint32)
    # three values that differ in every digit (a width of 1 bit has only two: the first and the last then coincide)
    three = np.array([top, 0x2AAAAAAA & top, 0x55555555 & top], np.uint32)
    i = np.arange(n)
    out = {
        "uniform": uniform,
        "all equal": np.full(n, 0x9E3779B9 & top, np.uint32),          # every pass takes the all-one-bin branch
        "three values, runs of 1000": three[(i // 1000) % 3],         # whole waves on one digit
        "three values, runs of 63": three[(i // 63) % 3],             # a run starts at every lane in turn, lanes 0 and 63 included
        "three values, interleaved": three[i % 3],
        "sorted": np.sort(uniform),
        "reverse sorted": np.sort(uniform)[::-1].copy(),
    }
    if nbits > 24:          # the depth-sort shape: a constant top byte over 24 random bits (at 24 bits and below that IS the uniform set)
        out["constant top byte"] = np.uint32(min(0x40, top >> 24) << 24) | rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32)
    return out


def run_sort(keys, vals, nbits, mode, kept=False, alt=False):
    """One radix_sort_pairs in `mode`; checks the return code and every guard, returns the host copies of the four buffers and the two words."""
    n = len(keys)
    elems = lib().ibgs_debug_sort_scratch_elems(n)
    k0, k1, v0, v1 = dev(keys), dev([], n), dev(vals), dev([], n)
    scratch = dev([], elems)          # not zeroed: the sort is told so (scratch_is_zero = false)
    kept_w, alt_w = dev([0]), dev([0])          # device words the caller zeroes (common.h)
    prev = lib().ibgs_debug_set_onesweep(mode)
    try:
        rc = lib().ibgs_debug_sort_pairs(stream(), k0.data_ptr(), k1.data_ptr(), v0.data_ptr(), v1.data_ptr(), n, nbits, scratch.data_ptr(), elems,
                                         kept_w.data_ptr() if kept else None, alt_w.data_ptr() if alt else None)
        torch.cuda.synchronize()
    finally:
        lib().ibgs_debug_set_onesweep(prev)
    assert rc == 0, _lib.last_error()
    r = {"k0": host(k0), "k1": host(k1), "v0": host(v0), "v1": host(v1), "kept": host(kept_w), "alt": host(alt_w)}
    for name in ("k0", "k1", "v0", "v1"):
        assert untouched(r[name][n:]), "wrote behind " + name
    assert untouched(host(scratch)[elems:]), "wrote behind the scratch"
    assert untouched(r["kept"][1:]) and untouched(r["alt"][1:])
    if not kept:
        assert r["kept"][0] == 0
    if not alt:
        assert r["alt"][0] == 0
    return r


def test_set_onesweep_returns_the_previous_mode():
    first = lib().ibgs_debug_set_onesweep(CLASSIC)
    try:
        assert lib().ibgs_debug_set_onesweep(SINGLE_LAUNCH) == CLASSIC
        assert lib().ibgs_debug_set_onesweep(BY_SIZE) == SINGLE_LAUNCH
        assert lib().ibgs_debug_set_onesweep(CLASSIC) == BY_SIZE
    finally:
        lib().ibgs_debug_set_onesweep(first)
    assert lib().ibgs_debug_set_onesweep(first) == first


@pytest.mark.parametrize("mode", MODES, ids=["classic", "single_launch"])
@pytest.mark.parametrize("n,nbits", SHAPES)
def test_sort_is_the_stable_sort(n, nbits, mode):
    vals = np.arange(n, dtype=np.uint32)
    for name, keys in key_sets(n, nbits).items():
        want_k, want_v = stable_reference(keys, vals)
        assert np.array_equal(want_k, np.sort(keys))
        r = run_sort(keys, vals, nbits, mode)
        assert np.array_equal(r["k0"][:n], want_k), name
        assert np.array_equal(r["v0"][:n], want_v), name


@pytest.mark.parametrize("mode", MODES, ids=["classic", "single_launch"])
@pytest.mark.parametrize("nbits", [13, 32])
def test_sort_carries_arbitrary_values(nbits, mode):
    """Random words as values (at 13 bits every key repeats ~37 times: the values tell whether equal keys kept their order)."""
    n = 300001
    keys = key_sets(n, nbits)["uniform"]
    vals = np.random.default_rng(5).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    want_k, want_v = stable_reference(keys, vals)
    r = run_sort(keys, vals, nbits, mode)
    assert np.array_equal(r["k0"][:n], want_k) and np.array_equal(r["v0"][:n], want_v)


@pytest.mark.parametrize("n", [CHUNK + 1, 300001])
def test_result_alt_names_the_buffer_that_holds_the_result(n):
    """32-bit keys, single-launch passes: a last pass that would move nothing leaves its input where it is (keys1 / vals1) and sets the word."""
    vals = np.arange(n, dtype=np.uint32)
    sets = key_sets(n, 32)
    for name, where in (("constant top byte", 1), ("uniform", 0)):
        want_k, want_v = stable_reference(sets[name], vals)
        r = run_sort(sets[name], vals, 32, SINGLE_LAUNCH, alt=True)
        assert r["alt"][0] == where, name
        named = int(r["alt"][0])
        assert np.array_equal(r["k%d" % named][:n], want_k), name
        assert np.array_equal(r["v%d" % named][:n], want_v), name


@pytest.mark.parametrize("mode", MODES, ids=["classic", "single_launch"])
@pytest.mark.parametrize("n", [CHUNK + 1, 300001])
def test_kept_dev_counts_and_sorts_the_other_keys(n, mode):
    """A share of the keys is 0xFFFFFFFF: *kept_dev = the number K of the others, the first K pairs are their stable sort.  What lies behind K is
    unspecified (common.h) and not looked at."""
    rng = np.random.default_rng(n + 17)
    vals = np.arange(n, dtype=np.uint32)
    for n_dropped in (0, n // 10, n - 1, n):
        keys = rng.integers(0, DROPPED, n, dtype=np.uint64).astype(np.uint32)          # below 0xFFFFFFFF
        keys[rng.permutation(n)[:n_dropped]] = DROPPED
        others = keys != DROPPED
        K = int(others.sum())
        assert K == n - n_dropped
        want_k, want_v = stable_reference(keys[others], vals[others])
        r = run_sort(keys, vals, 32, mode, kept=True)
        assert r["kept"][0] == K, n_dropped
        assert np.array_equal(r["k0"][:K], want_k), n_dropped
        assert np.array_equal(r["v0"][:K], want_v), n_dropped


def test_the_library_s_own_choice_at_the_first_classic_size():
    """n = 4096 chunks + 1 key: the first size at which the library itself (mode -1) takes the hist + scan + scatter passes; the histogram
    (128 bins x 4097 chunks) then needs a two-level scan.  20-bit keys: the deterministic backward's id sort at the benchmark's size -- three 7-bit
    passes and the copy-back.  ~270 MB of device memory.  The numpy reference (one sort of 16.8 M uint64) dominates this test's run time."""
    n, nbits = CHUNK * CHUNK + 1, 20
    keys = np.random.default_rng(20).integers(0, 1 << nbits, n, dtype=np.uint64).astype(np.uint32)
    vals = np.arange(n, dtype=np.uint32)
    want_k, want_v = stable_reference(keys, vals)
    r = run_sort(keys, vals, nbits, BY_SIZE)
    assert np.array_equal(r["k0"][:n], want_k)
    assert np.array_equal(r["v0"][:n], want_v)


@pytest.mark.parametrize("nbits", [13, 32])
def test_single_launch_passes_repeat_themselves(nbits):
    """The chunks are handed out by ticket, in an order that differs from run to run; no buffer may."""
    n = 300001
    keys = key_sets(n, nbits)["uniform"]
    vals = np.arange(n, dtype=np.uint32)
    a = run_sort(keys, vals, nbits, SINGLE_LAUNCH)
    b = run_sort(keys, vals, nbits, SINGLE_LAUNCH)
    for name in ("k0", "v0", "k1", "v1"):
        assert np.array_equal(a[name], b[name]), name
    want_k, want_v = stable_reference(keys, vals)
    assert np.array_equal(a["k0"][:n], want_k) and np.array_equal(a["v0"][:n], want_v)
