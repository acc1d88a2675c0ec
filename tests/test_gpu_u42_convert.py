"""The split six-bit planes' converts ALONE on the MI355X (kernels_scan42.h::u42_unpack8, ::u42_rem4), launched by
tests/kernel_harness/u42_convert_harness.hip.

The full pass reads a masked byte 0x0h, h in 0 .. 15, as OCP e4m3 and relies on the result being exactly h * 2^-9 -- the bytes
0 .. 7 are e4m3 SUBNORMALS -- so that P' = 2^-9 P bit for bit.  This table decides whether that holds under the library's
build flags: every nibble value in every nibble position, every remainder in every remainder position, compared bitwise."""
import numpy as np
import pytest

import u42_convert_harness as CH
import u42_harness as H

F32, U32 = np.float32, np.uint32


def _expect(values):
    """value * 2^-9 as fp32 bit patterns (exact: a four-bit integer times a power of two)"""
    want = (values.astype(F32) * F32(2.0 ** -9)).astype(F32)
    assert np.array_equal(want * F32(512.0), values.astype(F32))
    return want.view(U32)


def _nibble_table():
    """dwords [3 * 8 * 16] and their elements [.., 8]: value v in nibble position p over backgrounds of 0, of 15 and of a
    pattern that differs in every position"""
    rows = []
    for background in (np.zeros(8, U32), np.full(8, 15, U32), np.array([3, 12, 5, 10, 9, 6, 1, 14], U32)):
        for p in range(8):
            for v in range(16):
                e = background.copy()
                e[p] = v
                rows.append(e)
    return np.array(rows, U32)


def _remainder_table():
    rows = []
    for background in (np.zeros(16, U32), np.full(16, 3, U32), (np.arange(16, dtype=U32) * 7 + 1) % 4):
        for p in range(16):
            for v in range(4):
                e = background.copy()
                e[p] = v
                rows.append(e)
    return np.array(rows, U32)


def test_tables_cover_every_value_in_every_position():
    """CPU: the tables hold what the issue asks for, and the packers place them as the planes' layout says"""
    nib, rem = _nibble_table(), _remainder_table()
    assert {(p, int(v)) for p in range(8) for v in nib[:128, p]} == {(p, v) for p in range(8) for v in range(16)}
    assert {(p, int(v)) for p in range(16) for v in rem[:64, p]} == {(p, v) for p in range(16) for v in range(4)}
    # one dword of eight elements sits at dword 0 of a one-unit row of pack_h; sixteen remainders at dword 0 of pack_l
    e = np.full((1, 32), 8, U32)
    e[0, :8] = nib[300]
    assert np.array_equal(H.unpack_h(H.pack_h(e), 1)[0, :8], nib[300])
    r = np.zeros((1, 32), U32)
    r[0, :16] = rem[100]
    assert np.array_equal(H.unpack_l(H.pack_l(r, np.zeros(1, F32)), 1)[0][0, :16], rem[100])


def _pack_nibbles(elems):
    full = np.full((len(elems), 32), 8, U32)
    full[:, :8] = elems
    return np.array([H.pack_h(full[i:i + 1])[0, 0, 0, 0] for i in range(len(elems))], U32)


def _pack_remainders(elems):
    full = np.zeros((len(elems), 32), U32)
    full[:, :16] = elems
    return H.pack_l(full, np.zeros(len(elems), F32))[:, 0].copy()


@pytest.mark.gpu
def test_every_nibble_in_every_position_is_its_value_times_2_to_minus_9():
    elems = _nibble_table()
    got = CH.nibbles(_pack_nibbles(elems))
    want = _expect(elems)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(elems[i].tolist(), j, hex(got[i, j]), hex(want[i, j])) for i, j in bad[:4]]
    assert np.array_equal(got.view(F32) * F32(512.0), elems.astype(F32))


@pytest.mark.gpu
def test_every_remainder_in_every_position_is_its_value_times_2_to_minus_9():
    elems = _remainder_table()
    got = CH.remainders(_pack_remainders(elems))
    want = _expect(elems)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(elems[i].tolist(), j, hex(got[i, j]), hex(want[i, j])) for i, j in bad[:4]]
    assert np.array_equal(got.view(F32) * F32(512.0), elems.astype(F32))
