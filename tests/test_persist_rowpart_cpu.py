"""CPU: the addressing of the persistent solve's tile-major LayerNorm row partials (persist.hpp xpart_off / row_owner,
exported host-side as flamed_persist_rowpart; no GPU).  For dense and exact-lengths batches under both row partitions:
every (frame, slot) has one 8-B cell of its own inside the buffer, the 16 rows of a (group, tile, slot) fill exactly one
128-B-aligned line, rows past a group's end map nowhere, and the (group, row in group) that a reader derives for a
frame -- the depthwise halo reads other groups' rows that way -- is the one its writer used."""
import ctypes

import pytest

GROUPS, SLOTS, MAX_ROWS = 8, 32, 512
BUF = GROUPS * (MAX_ROWS // 16) * SLOTS * 128  # bytes of one partial buffer (persist.hpp kXpartBytes; independent of T)


@pytest.fixture(scope="module")
def lib():
    from flamed import _native
    return _native.lib()


def group_rows(g, T, Lu, B, opt):
    """persist.hip group_rows: the frames [r0, r0 + nr) of group g."""
    gpu = GROUPS // B
    u, gi = divmod(g, gpu)
    if opt & 2:
        MT = (Lu + 15) // 16
        tb, te = gi * MT // gpu, (gi + 1) * MT // gpu
        return u * T + 16 * tb, max(min(16 * te, Lu) - 16 * tb, 0)
    R = (Lu + gpu - 1) // gpu
    return u * T + gi * R, max(min(R, Lu - gi * R), 0)


def query(lib, B, T, lens, opt, g, lrow, s):
    row, og, ol, off = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    arr = (ctypes.c_int * B)(*lens) if lens else None
    assert lib.flamed_persist_rowpart(B, T, arr, opt, g, lrow, s, ctypes.byref(row), ctypes.byref(off), ctypes.byref(og),
                                      ctypes.byref(ol)) == 0
    return row.value, off.value, og.value, ol.value


CASES = [(1, 16, None), (1, 131, None), (1, 400, None), (4, 100, None), (2, 1111, None), (4, 100, [100, 61, 37, 16])]


@pytest.mark.parametrize("opt", [0, 2], ids=["equal-shares", "whole-tiles"])
@pytest.mark.parametrize("B,T,lens", CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_cells_distinct_lines_whole_and_owner_agrees(lib, B, T, lens, opt):
    gpu = GROUPS // B
    cells, frames = {}, set()
    for g in range(GROUPS):
        Lu = lens[g // gpu] if lens else T
        r0, nr = group_rows(g, T, Lu, B, opt)
        assert nr <= MAX_ROWS
        for lrow in range(nr):
            for s in (0, 1, 17, SLOTS - 1) if lrow % 16 else range(SLOTS):
                row, off, og, ol = query(lib, B, T, lens, opt, g, lrow, s)
                assert row == r0 + lrow
                assert (og, ol) == (g, lrow), "a reader of this frame would look in another cell than its writer filled"
                assert off % 8 == 0 and 0 <= off <= BUF - 8
                assert off not in cells, f"cell shared by {cells[off]} and {(row, s)}"
                cells[off] = (row, s)
                # the 16 rows of this (tile, slot) share one 128-B-aligned line, in row order
                line = query(lib, B, T, lens, opt, g, lrow - lrow % 16, s)[1]
                assert line % 128 == 0 and off == line + 8 * (lrow % 16)
            frames.add(r0 + lrow)
        for lrow in (nr, nr + 1, nr + 15, MAX_ROWS):  # past the group's end: nowhere
            assert query(lib, B, T, lens, opt, g, lrow, 0)[:2] == (-1, -1)
    want = {u * T + i for u in range(B) for i in range(lens[u] if lens else T)}
    assert frames == want, "the groups' rows are not exactly the batch's frames"


def test_bad_arguments(lib):
    out = [ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()]
    refs = [ctypes.byref(o) for o in out]
    assert lib.flamed_persist_rowpart(3, 100, None, 0, 0, 0, 0, *refs) != 0  # B not 1 / 2 / 4 / 8
    assert lib.flamed_persist_rowpart(1, 100, None, 0, 8, 0, 0, *refs) != 0  # group
    assert lib.flamed_persist_rowpart(1, 100, None, 0, 0, 0, 32, *refs) != 0  # slot
    assert lib.flamed_persist_rowpart(1, 100, None, 0, 0, 0, 0, None, refs[1], refs[2], refs[3]) != 0
