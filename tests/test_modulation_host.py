"""CPU tests of the modulation mapper's host side (the built library, no GPU call): the scaling constants, the
descriptor layout, the Python mapper's length check, and the one-ulp fact about the test helpers."""
import ctypes

import numpy as np
import pytest

from tests import modulation_ref as M
from tests.vectors import modulate as modulate_f64


def test_scaling_bit_patterns():
    """ldpc_hip_modulation_scaling and the Python get_modulation_scaling return the reference's six float32 values
    (modulation_mapper_lut_impl.cpp), which np.sqrt(np.float32(1) / np.float32(P)) reproduces; 0.0 for scheme 3."""
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_modulation as cm
    L = _lib.load()
    for mod, power in ((0, 2), (1, 2), (2, 2), (4, 10), (6, 42), (8, 170)):
        want = M.SCALING_BITS[mod]
        assert np.array([np.sqrt(np.float32(1) / np.float32(power))], np.float32).view(np.uint32)[0] == want
        assert np.array([L.ldpc_hip_modulation_scaling(mod)], np.float32).view(np.uint32)[0] == want, mod
        assert np.array([cm.get_modulation_scaling(mod)], np.float32).view(np.uint32)[0] == want, mod
        assert np.array([cm.modulation_mapper.get_modulation_scaling(cm.modulation_scheme(mod))],
                        np.float32).view(np.uint32)[0] == want, mod
    assert L.ldpc_hip_modulation_scaling(3) == 0.0 and cm.get_modulation_scaling(3) == 0.0
    assert L.ldpc_hip_modulation_scaling(-1) == 0.0 and L.ldpc_hip_modulation_scaling(10) == 0.0


def test_mod_desc_layout():
    from srsran_projectvtlmo_amd import _lib
    assert ctypes.sizeof(_lib.ModDesc) == 40
    assert _lib.ModDesc.nof_symbols.offset == 24 and _lib.ModDesc.modulation.offset == 32
    assert (_lib.SYM_CF32, _lib.SYM_CI8) == (0, 1)


def test_helper_differs_from_float64_formula_by_one_ulp():
    """The float32 table (float32(level) * float32 scaling) is not the float64 formula rounded: they agree on the
    (pi/2-)BPSK and QPSK schemes and differ, by at most one ulp, somewhere in each of 16/64/256-QAM. This pins the
    fact so that neither helper is "fixed" to match the other."""
    for mod in M.SCHEMES:
        bits = M.all_index_bits(mod)
        a, b = M.modulate(bits, mod), modulate_f64(bits, mod)
        ua, ub = a.view(np.uint32).astype(np.int64), b.view(np.uint32).astype(np.int64)
        if mod in (0, 1, 2):
            assert np.array_equal(ua, ub), mod
        else:
            assert not np.array_equal(ua, ub), mod
            assert np.abs(ua - ub).max() == 1, mod


def test_helper_levels_are_the_nested_forms():
    """The integer levels: odd, within +-(2^(Qm/2) - 1), every constellation point exactly once, unit mean power after
    scaling."""
    for mod in (2, 4, 6, 8):
        lv = M.levels(M.all_index_bits(mod), mod).astype(np.int32)
        top = (1 << (mod // 2)) - 1
        assert np.all(lv % 2 != 0) and lv.min() == -top and lv.max() == top
        assert len({(int(r), int(i)) for r, i in lv}) == 1 << mod
        assert abs(float((lv.astype(np.float64) ** 2).sum(axis=1).mean()) * float(M.scaling(mod)) ** 2 - 1) < 1e-6
    assert M.levels([0, 0, 1, 1], 1).tolist() == [[1, 1], [1, 1], [-1, -1], [-1, -1]]
    assert M.levels([0, 0, 1, 1], 0).tolist() == [[1, 1], [-1, 1], [-1, -1], [1, -1]]
    assert M.levels([1, 0, 1, 1], 4).tolist() == [[-3, 3]]        # s = (-1, 1, -1, -1): (s0 (2 - s2), s1 (2 - s3))
    assert M.levels([0, 1, 0, 0, 1, 0], 6).tolist() == [[1, -3]]  # (s0 (4 - s2 (2 - s4)), s1 (4 - s3 (2 - s5)))


def test_python_mapper_length_check():
    """modulate raises ValueError on the reference's assert (bits != Qm x symbols) before any GPU call."""
    from srsran_projectvtlmo_amd import channel_modulation as cm

    class no_ctx:
        handle = None
    mapper = cm.modulation_mapper_hip(no_ctx())
    with pytest.raises(ValueError):
        mapper.modulate(np.zeros(5, np.complex64), np.zeros(2, np.uint8), cm.modulation_scheme.QAM16, nof_bits=16)
    with pytest.raises(ValueError):
        mapper.modulate(np.zeros(4, np.complex64), np.zeros(3, np.uint8), cm.modulation_scheme.QAM16)
    with pytest.raises(ValueError):
        mapper.modulate(np.zeros((4, 3), np.int8), np.zeros(2, np.uint8), cm.modulation_scheme.QAM16)
    with pytest.raises(ValueError):
        mapper.modulate(np.zeros(4, np.float32), np.zeros(2, np.uint8), cm.modulation_scheme.QAM16)
    assert hasattr(cm.channel_modulation_factory, "create_modulation_mapper")
