"""CPU tests of the pseudo-random sequence generator's host side (ldpc_hip_prs_init: an O(log offset) jump) against the
brute-force walk of the TS 38.211 5.2.1 recurrences (tests/scrambling_ref.py), pinned known answers, and the slot
pipeline's per-codeblock scrambling descriptors. No GPU call is made here."""
import ctypes

import numpy as np
import pytest

from tests import scrambling_ref as R

C_INITS = [0, 1, 0x7FFFFFFF, 0x091A0155]  # the last: rnti 0x1234, n_id 0x155
OFFSETS = [0, 1, 31, 32, 1599, 1600, 32767, 32768, 32769, 100000, (1 << 24) + 5]


def _prs_init(c_init, offset):
    from srsran_projectvtlmo_amd import _lib
    st = _lib.PrsState()
    assert _lib.load().ldpc_hip_prs_init(c_init, offset, ctypes.byref(st)) == _lib.OK
    return int(st.x1), int(st.x2)


def test_reference_walks_agree():
    """The reference's fast walk (squared recurrences) equals the recurrences walked exactly as written."""
    for c_init in C_INITS:
        plain = R.walk_registers(c_init, 70000, plain=True)
        fast = R.walk_registers(c_init, 70000, plain=False)
        assert np.array_equal(plain[0], fast[0]) and np.array_equal(plain[1], fast[1])


@pytest.mark.parametrize("c_init", C_INITS)
def test_prs_init_matches_brute_force(c_init):
    for offset in OFFSETS:
        assert _prs_init(c_init, offset) == R.state(c_init, offset), f"offset {offset}"


def test_prs_init_known_answers():
    assert R.state(0, 0)[0] == 0x5E485840
    assert _prs_init(0, 0)[0] == 0x5E485840
    assert _prs_init(0x091A0155, 0)[0] == 0x5E485840  # x1 does not depend on c_init
    known = [(0, 0, "021a127a25950356"), (1, 0, "028303742b9afde2"), (0x091A0155, 0, "71d93dbdaf346183"),
             (0x091A0155, 100000, "04cee0ed2ebe6d2a"), (0x7FFFFFFF, 3, "e85f9c717302bc76")]
    for c_init, offset, first64 in known:
        assert R.packed(c_init, offset, 64).tobytes().hex() == first64
        # the same 64 bits from the library's states: bit i of x1 ^ x2 is c(offset + i), i < 31
        bits = []
        for o in (offset, offset + 31, offset + 62):
            x1, x2 = _prs_init(c_init, o)
            bits += [((x1 ^ x2) >> i) & 1 for i in range(31)]
        assert np.packbits(np.array(bits[:64], np.uint8)).tobytes().hex() == first64


def test_prs_init_rejects_bad_arguments():
    from srsran_projectvtlmo_amd import _lib
    L = _lib.load()
    st = _lib.PrsState()
    assert L.ldpc_hip_prs_init(0x80000000, 0, ctypes.byref(st)) == _lib.EINVAL  # c_init is 31 bits
    assert L.ldpc_hip_prs_init(1, 0, None) == _lib.EINVAL


def test_python_state_follows_advance():
    from srsran_projectvtlmo_amd import sequence_generators as sg
    g = sg.create_pseudo_random_generator_hip_factory().create()
    g.init(sg.pusch_c_init(0x1234, 0x155))
    g.advance(1599)
    g.advance(1)
    st = g.get_state()
    assert (st.x1, st.x2) == R.state(0x091A0155, 1600)
    h = sg.pseudo_random_generator_hip()
    h.init(st)
    h.advance(31167)
    assert (h.get_state().x1, h.get_state().x2) == R.state(0x091A0155, 32767)


def test_slot_scramble_descriptors():
    """Cumulative sequence offsets per TB (unequal E), none for rnti = -1."""
    from srsran_projectvtlmo_amd import pusch
    from srsran_projectvtlmo_amd import sequence_generators as sg
    a = pusch.tb_slot_spec(20000, 1, 384, 0, [3000, 3000, 3006], 6, rnti=0x1234, n_id=0x155)
    b = pusch.tb_slot_spec(256, 2, 36, 0, [624], 2)
    c = pusch.tb_slot_spec(256, 2, 36, 0, [624, 630], 2, rnti=7, n_id=1023)
    assert b.rnti == -1 and b.n_id == 0
    e = pusch.slot_scramble_entries([a, b, c])
    assert e == [(0x091A0155, 0), (0x091A0155, 3000), (0x091A0155, 6000), None, (7 * 32768 + 1023, 0),
                 (7 * 32768 + 1023, 624)]
    assert pusch.slot_scramble_entries([b]) == [None]
    arr = sg.scramble_descriptors(e)
    assert [(d.c_init, d.enable, d.seq_offset) for d in arr] == [
        (0x091A0155, 1, 0), (0x091A0155, 1, 3000), (0x091A0155, 1, 6000), (0, 0, 0), (230399, 1, 0), (230399, 1, 624)]
