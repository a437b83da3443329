"""GPU: the stable segmented radix argsort (csrc/sort.hip: falnet_sort_u32, fal_net_amd/sparsification.py: argsort_u32) against
np.argsort(kind="stable") per segment, with torch.equal: a permutation has no tolerance.  Every output sits in a buffer pre-filled with 0xFF
with a guard region behind it.  The device path is compared with itself only where the property IS self-agreement (two calls)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import sparsification as SP  # noqa: E402

DEV = "cuda"
# one lane, around a wave, around a workgroup round, around a tile of 2048, and 257 tiles: 65792 table entries, more than one 4096-entry scan step
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2048 * 256 + 1]
FAMILIES = ["random", "equal", "two", "ascending", "descending", "top-byte", "bottom-byte"]
SEGMENTS = [1, 3, 8]
GUARD = 256  # int32 words behind perm


@functools.lru_cache(maxsize=None)
def family(name, n, row):
    """Segment `row` of a key family: n uint32 keys, seeded, computed once and left unchanged."""
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + row)
    if name == "random":
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    elif name == "equal":
        k = np.full(n, 0xDEADBEEF + row, np.uint64)
    elif name == "two":
        k = rng.choice(np.array([0x80000001, 5], np.uint64), n)
    elif name in ("ascending", "descending"):
        k = np.arange(n, dtype=np.uint64) * np.uint64(0xFFFFFFFF) // np.uint64(max(n, 1))  # over all four bytes
        k = k[::-1] if name == "descending" else k
    elif name == "top-byte":
        k = (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(24)) | np.uint64(0x00ABCDEF)
    else:
        k = np.uint64(0x12345600) | rng.integers(0, 256, n, dtype=np.uint64)
    k = np.ascontiguousarray(k.astype(np.uint32))
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def reference(name, n, row):
    return np.argsort(family(name, n, row), kind="stable").astype(np.int32)


def to_dev(keys_np):
    return torch.from_numpy(np.ascontiguousarray(keys_np).view(np.int32).copy()).to(DEV)


def raw_sort(keys_t, n, segments, tag):
    """falnet_sort_u32 into a 0xFF-filled buffer with a guard behind it -> the (segments, n) int32 permutation; the guard is checked here."""
    lib = L.lib()
    buf = torch.full((segments * n + GUARD,), -1, dtype=torch.int32, device=DEV)
    ws = torch.full((max(int(lib.falnet_sort_u32_workspace_bytes(n, segments)) // 8, 1) + 8,), -1, dtype=torch.int64, device=DEV)
    L.check(lib.falnet_sort_u32(L.ptr(keys_t), n, segments, L.ptr(buf), L.ptr(ws), L.stream_ptr()), "sort_u32")
    torch.cuda.synchronize()
    assert bool((buf[segments * n:] == -1).all()), tag + ": written behind perm"
    assert bool((ws[-8:] == -1).all()), tag + ": written behind the workspace"
    return buf[:segments * n].view(segments, n)


def check(rows_np, want_np, tag):
    segments, n = len(rows_np), len(rows_np[0])
    keys_np = np.stack(rows_np) if n else np.zeros((segments, 0), np.uint32)
    keys_t = to_dev(keys_np) if n else torch.zeros(8, dtype=torch.int32, device=DEV)  # n = 0: a pointer that is not NULL
    before = keys_t.clone()
    got = raw_sort(keys_t, n, segments, tag)
    want = torch.from_numpy(np.stack(want_np).reshape(segments, n))
    wrong = int((got.cpu() != want).sum())
    print(f"{tag}: {segments} x {n}, {wrong} ranks differ")
    assert torch.equal(got.cpu(), want), tag
    assert torch.equal(keys_t, before), tag + ": keys modified"
    again = raw_sort(keys_t, n, segments, tag)
    assert torch.equal(got, again), tag + ": two calls differ"
    return got


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_argsort_equals_numpy_stable(n, name):
    for segments in SEGMENTS:
        check([family(name, n, r) for r in range(segments)], [reference(name, n, r) for r in range(segments)], f"{name} n={n} segments={segments}")


@pytest.mark.parametrize("n", SIZES)
def test_segments_of_different_families_in_one_call(n):
    names = FAMILIES + ["random"]
    rows = [family(k, n, 7 - i) for i, k in enumerate(names)]
    check(rows, [reference(k, n, 7 - i) for i, k in enumerate(names)], f"mixed n={n}")


def test_equal_keys_keep_index_order_and_the_top_bit_is_unsigned():
    n = 5000
    got = check([family("equal", n, 0)], [np.arange(n, dtype=np.int32)], "all equal")
    assert torch.equal(got[0].cpu(), torch.arange(n, dtype=torch.int32))
    keys = np.array([0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, 0, 0x80000000, 1], np.uint32)  # as int32 the first would sort below the second
    check([keys], [np.array([3, 5, 1, 0, 4, 2], np.int32)], "unsigned order")


def test_public_wrapper_shapes_and_types():
    k2 = np.stack([family("random", 3000, r) for r in range(3)])
    want = torch.from_numpy(np.stack([reference("random", 3000, r) for r in range(3)]))
    t = to_dev(k2)
    got = SP.argsort_u32(t)
    assert got.dtype == torch.int32 and got.shape == t.shape and got.is_cuda and torch.equal(got.cpu(), want)
    assert torch.equal(SP.argsort_u32(t[1]).cpu(), want[1])  # (n,)
    if hasattr(torch, "uint32"):
        assert torch.equal(SP.argsort_u32(t.view(torch.uint32)).cpu(), want)
    assert tuple(SP.argsort_u32(t[:, :0].contiguous()).shape) == (3, 0)
    assert torch.equal(SP.argsort_u32(t.t().contiguous().t()).cpu(), want)  # a non-contiguous view is copied, not misread
    for bad in (t.float(), t.view(1, 3, 3000), torch.zeros((9, 4), dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError):
            SP.argsort_u32(bad)


def test_every_refusal_returns_nonzero_and_writes_nothing():
    lib = L.lib()
    n, segments = 3000, 3
    keys = to_dev(np.stack([family("random", n, r) for r in range(segments)]))
    buf = torch.full((segments * n + GUARD,), -1, dtype=torch.int32, device=DEV)
    ws = torch.full((int(lib.falnet_sort_u32_workspace_bytes(n, segments)) // 8 + 8,), -1, dtype=torch.int64, device=DEV)
    odd_perm, odd_ws = L.C.c_void_p(buf.data_ptr() + 4), L.C.c_void_p(ws.data_ptr() + 4)
    cases = [("n > 2^24", (L.ptr(keys), (1 << 24) + 1, 1, L.ptr(buf), L.ptr(ws)), r"2\^24"), ("n < 0", (L.ptr(keys), -5, 1, L.ptr(buf), L.ptr(ws)), r"2\^24"),
             ("0 segments", (L.ptr(keys), n, 0, L.ptr(buf), L.ptr(ws)), "segments"), ("9 segments", (L.ptr(keys), n, 9, L.ptr(buf), L.ptr(ws)), "segments"),
             ("null keys", (None, n, segments, L.ptr(buf), L.ptr(ws)), "null"), ("null perm", (L.ptr(keys), n, segments, None, L.ptr(ws)), "null"),
             ("null workspace", (L.ptr(keys), n, segments, L.ptr(buf), None), "null"), ("misaligned perm", (L.ptr(keys), n, segments, odd_perm, L.ptr(ws)), "8-byte"),
             ("misaligned workspace", (L.ptr(keys), n, segments, L.ptr(buf), odd_ws), "8-byte")]
    for tag, args, word in cases:
        rc = lib.falnet_sort_u32(*args, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0, tag
        with pytest.raises(RuntimeError, match=word):
            L.check(rc, "sort_u32")
        assert bool((buf == -1).all()) and bool((ws == -1).all()), tag  # nothing ran
    assert lib.falnet_sort_u32(L.ptr(keys), 0, segments, L.ptr(buf), L.ptr(ws), L.stream_ptr()) == 0  # n = 0: returns 0 ...
    torch.cuda.synchronize()
    assert bool((buf == -1).all()) and bool((ws == -1).all())  # ... and writes nothing
    assert lib.falnet_sort_u32(L.ptr(keys), n, segments, L.ptr(buf), L.ptr(ws), L.stream_ptr()) == 0  # and the next valid call is correct
    want = torch.from_numpy(np.stack([reference("random", n, r) for r in range(segments)]))
    assert torch.equal(buf[:segments * n].view(segments, n).cpu(), want) and bool((buf[segments * n:] == -1).all()) and bool((ws[-8:] == -1).all())
