"""The host schedule of the exact-fp32 tile GEMM (gemmt.hip), read through s3enc_debug_gemm_schedule — no device is touched.

A launch covers every batch's M x N with a bulk region of 64 tm-row tiles and, where "gemm32_tail" asks for one, a tail region of
64-row tiles that every XCD's range of workgroups ends with (the last workgroups dispatched).  The list the entry point returns is
built by the kernel's own block -> tile function, so what is checked here is the map the device runs."""

import ctypes as C

import pytest

N_VALUES = (128, 132, 256)
CU_COUNTS = (8, 104, 256, 304)
_BUF = (C.c_int32 * (4 * 4096))()


def _lib():
    from s3prl_amd import _lib

    return _lib, _lib.load()


def _schedule(lib, M, N, batches, tm, tail, cus):
    n = C.c_int64(0)
    rc = lib.s3enc_debug_gemm_schedule(M, N, batches, tm, tail, cus, _BUF, 4096, C.byref(n))
    assert rc == 0, lib.s3enc_last_error()
    assert 0 < n.value <= 4096
    flat = _BUF[: 4 * n.value]
    return list(zip(flat[0::4], flat[1::4], flat[2::4], flat[3::4])), n.value


def _todays_map(M, N, batches, tm):
    """The one-sequence XCD-aware map of a launch without a tail: every XCD (workgroup & 7) owns a contiguous range of the
    (batch, m-tile, n-tile) sequence, n fastest."""
    bm = 64 * tm
    nt, mt = (N + 127) // 128, (M + bm - 1) // bm
    nwg = nt * mt * batches
    q8, r8 = nwg >> 3, nwg & 7
    items = []
    for wg in range(nwg):
        xcd, loc = wg & 7, wg >> 3
        tile = (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + loc
        tn, tmb = tile % nt, tile // nt
        m0 = (tmb % mt) * bm
        items.append((tmb // mt, m0, min(bm, M - m0), tn * 128))
    return items


def _check(items, today, grid, M, N, batches, tm):
    """Partition, region shapes and dispatch order of one launch; returns the first row of the tail region (M when empty)."""
    bm = 64 * tm
    nt = (N + 127) // 128
    assert len(items) == grid and len(set(items)) == grid
    # the m-tiles, identical for every (batch, n-tile), cover [0, M) exactly once
    cols = {}
    for b, m0, rows, n0 in items:
        cols.setdefault((b, n0), []).append((m0, rows))
    assert sorted(cols) == [(b, 128 * t) for b in range(batches) for t in range(nt)]
    first = sorted(cols[(0, 0)])
    at = 0
    for m0, rows in first:
        assert m0 == at and rows > 0
        at += rows
    assert at == M
    for v in cols.values():
        assert sorted(v) == first
    assert grid == len(first) * nt * batches  # the launch's grid: (bulk + tail m-tiles) x n-tiles x batches
    # the tail region: the trailing run of m-tiles of at most 64 rows (of a launch of taller tiles)
    k = len(first)
    if tm > 1:
        while k > 0 and first[k - 1][1] <= 64:
            k -= 1
    tail_row = first[k][0] if k < len(first) else M
    for m0, rows in first[:k]:  # bulk: whole tiles on the bulk pitch (the last may be ragged when there is no tail)
        assert m0 % bm == 0 and (rows == bm or (m0 + rows == M and tail_row == M))
    for m0, rows in first[k:]:  # tail: 64 rows, or the ragged remainder
        assert (m0 - tail_row) % 64 == 0 and (rows == 64 or m0 + rows == M)
    # within every XCD's range of workgroups (wg & 7, ascending) all bulk items precede all tail items.  (A launch WITHOUT a tail
    # whose last bulk tile is ragged and at most 64 rows has the same m-tiles as one with a one-tile tail: it is today's list.)
    for xcd in range(8 if items != today else 0):
        seen_tail = False
        for b, m0, rows, n0 in items[xcd::8]:
            if m0 >= tail_row:
                seen_tail = True
            else:
                assert not seen_tail, "a bulk tile is dispatched behind a tail tile of its XCD"
    return tail_row


@pytest.mark.parametrize("batches", [1, 3])
@pytest.mark.parametrize("N", N_VALUES)
def test_schedule_partitions_the_output_and_ends_every_xcd_range_with_the_tail(N, batches):
    _, lib = _lib()
    with_tail = 0
    for M in range(1, 1101):
        for tm in (1, 2, 3, 4):
            bm = 64 * tm
            today = _todays_map(M, N, batches, tm)
            for cus in CU_COUNTS:
                # key 0: today's launches exactly
                items, grid = _schedule(lib, M, N, batches, tm, 0, cus)
                assert items == today, (M, N, batches, tm, cus)
                # key 2: the largest tail M allows — one bulk tile where M holds more than one, else none
                items, grid = _schedule(lib, M, N, batches, tm, 2, cus)
                tail_row = _check(items, today, grid, M, N, batches, tm)
                if tm > 1 and M > 64:
                    assert tail_row == (bm if M > bm else 0), (M, N, batches, tm, tail_row)
                elif tm == 1:
                    assert items == today
                # key 1: by shape
                items, grid = _schedule(lib, M, N, batches, tm, 1, cus)
                tail_row = _check(items, today, grid, M, N, batches, tm)
                slots = cus * {1: 4, 2: 4, 3: 3, 4: 2}[tm]
                if tm == 1 or len(today) < slots or len(today) % slots == 0:
                    assert items == today, "no tail without a whole round and a remainder behind it"
                elif items != today:
                    with_tail += 1
                    assert tail_row % bm == 0 and tail_row * ((N + 127) // 128) * batches // bm <= (len(today) // slots) * slots, \
                        "the bulk must fit the whole rounds"
    if N == 256 and batches == 3:  # up to 54 tiles of 128 rows: more than a round of the 8-CU part's 32 slots
        assert with_tail > 0, "the shape rule never chose a tail on the 8-CU part"


def test_schedule_entry_point_rejects_bad_arguments():
    _, lib = _lib()
    n = C.c_int64(0)
    assert lib.s3enc_debug_gemm_schedule(0, 128, 1, 2, 1, 256, None, 0, C.byref(n)) != 0
    assert lib.s3enc_debug_gemm_schedule(64, 128, 1, 5, 1, 256, None, 0, C.byref(n)) != 0
    assert lib.s3enc_debug_gemm_schedule(64, 128, 1, 2, 3, 256, None, 0, C.byref(n)) != 0
    assert lib.s3enc_debug_gemm_schedule(64, 128, 1, 2, 1, 256, None, 0, None) != 0
    assert lib.s3enc_debug_gemm_schedule(300, 256, 2, 2, 0, 256, None, 0, C.byref(n)) == 0 and n.value == 3 * 2 * 2  # count only
