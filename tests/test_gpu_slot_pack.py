"""slot_pack_kernel / slot_unpack_kernel alone (csrc/snapshot/slot_pack.hip through sva_test_slot_pack) against a numpy gather and scatter.

A synthetic arena of 3 slots holds one segment of every shape at which the kernels take another arm: rows of 1, 3, 4, 5 and 68 elements of
2 and 4 bytes, strided (the element-wise arm at row ends) and contiguous; bases misaligned to 16 bytes; two rings (4-byte elements advancing
one element per step, 2-byte elements advancing 8) at rotation 0, mid-ring and N - 1 (a wrapping row); a KV prefix of 1 row and of all
S = 8 rows; a blocked plane of two 32-k blocks; a zero-row segment; a 12 KB contiguous segment so that the image spans several workgroups.
The image must equal the numpy image byte for byte, zero padding included (the hook pre-fills it with 0xA5), and after the unpack into
another slot at another ring rotation every byte of the destination arena outside that slot's rows -- the other slots, the gaps behind
every row and every segment -- must still be the sentinel that was uploaded.  Exact comparison: the kernels only move bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SLOTS = 3
PLAIN, RING, KV, BLOCKED = 0, 1, 2, 3


def _table(kv_rows):
    """[(rows, row elements, row stride elements, elem bytes, kind, ring_step, misalign bytes, rows allocated)]"""
    segs = []
    for elem in (2, 4):
        for n in (1, 3, 4, 5, 68):
            segs.append((3, n, n + 3, elem, PLAIN, 0, elem, 3))          # strided rows, base off 16-byte alignment
        segs.append((2, 68, 68, elem, PLAIN, 0, 0, 2))                   # contiguous rows, aligned base: the 16-byte arm
        segs.append((2, 5, 5, elem, PLAIN, 0, 4, 2))                     # contiguous rows whose payload is no multiple of 16
    segs.append((1, 37, 37, 4, RING, 1, 4, 1))
    segs.append((1, 40, 40, 2, RING, 8, 0, 1))
    for elem in (2, 4):
        for _ in range(2):                                              # two (layer, head) pieces of a cache with S = 8 rows
            segs.append((kv_rows, 64, 64, elem, KV, 0, 0, 8))
    for _ in range(2):                                                  # one plane, two 32-k blocks: 6 history rows of 32 unsigned shorts each
        segs.append((6, 32, 32, 2, BLOCKED, 0, 0, 6))
    segs.append((0, 16, 16, 4, PLAIN, 0, 0, 1))                          # a zero-row segment
    segs.append((1, 3000, 3000, 4, PLAIN, 0, 8, 1))                      # several workgroups
    segs.append((1, 1, 1, 4, PLAIN, 0, 12, 1))                           # a scalar (d_last_pos ...)
    return segs


def _build(kv_rows):
    table, off = [], 32
    for rows, n, stride, elem, kind, ring_step, mis, rows_alloc in _table(kv_rows):
        off = (off + 15) // 16 * 16 + mis
        slot_stride = (rows_alloc * stride + 5) * elem                   # a gap of 5 elements behind every slot's rows
        table.append([off, off, slot_stride, stride * elem, n * elem, rows, kind, elem, ring_step])
        off += N_SLOTS * slot_stride + 24
    return np.array(table, dtype=np.int64), off + 64


def _origin(seg, step):
    _, _, _, _, row_bytes, _, kind, elem, ring_step = (int(v) for v in seg)
    return (step * ring_step) % (row_bytes // elem) * elem if kind == RING else 0


def _np_pack(table, arena, slot, step):
    out = []
    for seg in table:
        off, _, ss, rs, rb, rows, kind, elem, _ = (int(v) for v in seg)
        o = _origin(seg, step)
        payload = [np.roll(arena[off + slot * ss + r * rs:off + slot * ss + r * rs + rb], -o) for r in range(rows)]
        p = np.concatenate(payload) if payload else np.zeros(0, np.uint8)
        out.append(np.concatenate([p, np.zeros(-p.size % 16, np.uint8)]))
    return np.concatenate(out)


def _np_unpack(table, arena, image, slot, step):
    arena = arena.copy()
    pos = 0
    for seg in table:
        _, off, ss, rs, rb, rows, kind, elem, _ = (int(v) for v in seg)
        o = _origin(seg, step)
        for r in range(rows):
            arena[off + slot * ss + r * rs:off + slot * ss + r * rs + rb] = np.roll(image[pos + r * rb:pos + (r + 1) * rb], o)
        pos += (rows * rb + 15) // 16 * 16
    return arena


@pytest.mark.parametrize("kv_rows", [1, 8])
@pytest.mark.parametrize("steps", [(0, 36), (18, 0), (36, 18)], ids=["rot0_to_last", "mid_to_0", "last_to_mid"])
@pytest.mark.parametrize("slots", [(0, 2), (2, 0)], ids=["first_to_last", "last_to_first"])
def test_pack_unpack_against_numpy(slots, steps, kv_rows):
    from streamvoiceanon_amd import engine as E

    table, nbytes = _build(kv_rows)
    rng = np.random.default_rng(100 * kv_rows + steps[0])
    src = rng.integers(1, 256, nbytes, dtype=np.uint8)
    dst = np.full(nbytes, 0x5A, np.uint8)                                # sentinels everywhere in the destination
    want_img = _np_pack(table, src, slots[0], steps[0])
    assert want_img.size > 3 * 4096 and want_img.size % 16 == 0
    img, got = E.test_slot_pack(table, src, dst, slots[0], slots[1], step_src=steps[0], step_dst=steps[1], cus=2)
    np.testing.assert_array_equal(img, want_img, err_msg="image (zero padding included)")
    want = _np_unpack(table, dst, want_img, slots[1], steps[1])
    np.testing.assert_array_equal(got, want, err_msg="destination arena after the unpack")
    # the model itself: everything outside the destination slot's rows is still the sentinel, and a round trip restores the source's rows
    touched = want != 0x5A
    assert touched.sum() <= want_img.size and (got[~touched] == 0x5A).all()
    np.testing.assert_array_equal(_np_pack(table, got, slots[1], steps[1]), want_img)


def test_a_table_that_leaves_the_arena_is_refused():
    from streamvoiceanon_amd import engine as E

    table, nbytes = _build(1)
    src, dst = np.ones(nbytes, np.uint8), np.ones(nbytes, np.uint8)
    bad = table.copy()
    bad[-2, 0] = nbytes - 64                                             # the 12 KB segment would run past the source arena
    with pytest.raises(RuntimeError, match="leaves the source arena"):
        E.test_slot_pack(bad, src, dst, 0, 1)
    bad = table.copy()
    bad[0, 7] = 3
    with pytest.raises(RuntimeError, match="bad segment"):
        E.test_slot_pack(bad, src, dst, 0, 1)
