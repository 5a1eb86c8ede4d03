"""Where the one-launch tCG run (k_tcg_run) keeps its residual image in LDS, enumerated on the CPU.

dcora_debug_run_image returns what the kernel itself uses: the byte offset of every pair of doubles of the image
(run_img_off) and the logical lane of each of a wave's 64 lanes in the product (wg_sums_logical_lane).  From them the
test rebuilds every 16-byte LDS access of the image and checks it against the way the LDS serves it: ds_read_b128 takes
16 lanes per cycle, in the groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, over 64 banks of 4
bytes -- sixteen 16-byte slots per 256-byte row; two lanes of a group on one slot cost a cycle each.

A rank listed in PADDED carries pads in its image, and every read and every staging write of it must be free of
conflicts.  No rank is listed today: the padding of r = 5 (one 16-byte pad behind every 160 pairs) passed these checks
and was measured slower than the plain image (profiles/run_image.txt); the pad r = 4 and r = 6 would need, one per 2
lanes' blocks, falls inside the 16 consecutive pairs that 16 consecutive threads write.  For the plain images the map
and the writes are checked and the reads' conflicts are printed (r = 4: 8-way, r = 5: 2-way, r = 6: 4-way)."""
import ctypes

import numpy as np
import pytest

WG = 256
GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
          [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS = GROUPS + [[p + 32 for p in g] for g in GROUPS]
PADDED = ()
SIZES = [132, 644, 2000, 2048]


def _image(r, k):
    from dcora_amd import capi
    cpad = (k + 127) // 128 * 128
    off = np.full(cpad * r // 2, -1, dtype=np.int32)
    lanes = np.full(64, -1, dtype=np.int32)
    nbytes = ctypes.c_int(-1)
    assert capi.lib().dcora_debug_run_image(r, k, off, lanes, ctypes.byref(nbytes)) == 0
    return cpad, off.astype(np.int64), lanes.astype(np.int64), nbytes.value


def _slots(off):
    return (off // 16) % 16


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("r", [4, 5, 6])
def test_image_map_is_an_aligned_bijection_into_the_allocation(built, r, k):
    cpad, off, lanes, nbytes = _image(r, k)
    assert sorted(lanes.tolist()) == list(range(64)), lanes
    assert np.all(off >= 0) and np.all(off % 16 == 0)
    assert len(np.unique(off)) == len(off) == cpad * r // 2
    nbytes -= 16                                             # (behind the image: the spare pair of the update)
    assert off.max() + 16 <= nbytes, (off.max(), nbytes)
    assert np.all(np.diff(off) >= 16)                        # ascending: a pad only ever moves what follows it
    grow = nbytes / (cpad * r * 8.0) - 1.0
    print("r %d k %d: %d bytes of LDS, %.2f %% above the plain image" % (r, k, nbytes, 100 * grow))
    assert nbytes <= 128 * 1024
    assert grow <= (0.007 if r in PADDED else 0.0)
    # a lane's r pairs of a step are contiguous: the kernel reads them at the first one's offset + 16 tq
    first = off[::r]
    for tq in range(r):
        assert np.array_equal(off[tq::r], first + 16 * tq)


def _read_conflicts(r, k):
    """the worst number of lanes of one service group on one 16-byte slot, over every step, tq and group"""
    cpad, off, lanes, _ = _image(r, k)
    worst = 0
    for sidx in range(cpad // 128):
        for tq in range(r):
            for g in GROUPS:
                pairs = (sidx * 64 + lanes[g]) * r + tq
                assert len(set(pairs.tolist())) == 16
                worst = max(worst, int(np.bincount(_slots(off[pairs]), minlength=16).max()))
    return worst


def _write_conflicts(r, k):
    """staging, zero fill and update: thread e of 256 writes pair u * 256 + e; 16 consecutive threads at a time"""
    cpad, off, _, _ = _image(r, k)
    npairs, worst = cpad * r // 2, 0
    assert npairs % 16 == 0
    for i0 in range(0, npairs, 16):
        worst = max(worst, int(np.bincount(_slots(off[i0:i0 + 16]), minlength=16).max()))
    return worst


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("r", [4, 5, 6])
def test_product_reads_and_staging_writes_hit_sixteen_distinct_slots(built, r, k):
    """every service group of every product read (all steps, all tq) and every 16 consecutive threads of a write hit 16
    distinct 16-byte slots where the image is padded; the plain images' reads are printed, not judged."""
    rd, wr = _read_conflicts(r, k), _write_conflicts(r, k)
    print("r %d k %d: product reads %d-way, writes %d-way" % (r, k, rd, wr))
    assert wr == 1, wr
    if r in PADDED:
        assert rd == 1, rd
