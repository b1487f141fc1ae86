"""CPU reference of the modulation mapper as the reference computes it (modulation_mapper_lut_impl.cpp), in integers
and float32 numpy, written from the rule:

    symbol i takes bits b0 .. b(Qm-1) = input bits Qm i .. Qm i + Qm - 1;  s_k = 1 - 2 b_k
    Re from the even-index bits, Im from the odd ones, in the nested form of TS 38.211 5.1:
      QPSK (s0, s1); 16-QAM (s0 (2 - s2), s1 (2 - s3)); 64-QAM (s0 (4 - s2 (2 - s4)), s1 (4 - s3 (2 - s5)));
      256-QAM (s0 (8 - s2 (4 - s4 (2 - s6))), s1 (8 - s3 (4 - s5 (2 - s7)))); BPSK (s0, s0);
      pi/2-BPSK (s0, s0) at even symbol positions of the span and (-s0, s0) at odd ones
    ci8 = these odd integers; cf32 = float32(level) * scaling, one float32 multiply per component

The six scalings are pinned as bit patterns: 1/sqrt(2), sqrtf(1.0f / 10), sqrtf(1.0f / 42), sqrtf(1.0f / 170), which
np.sqrt(np.float32(1) / np.float32(P)) reproduces. The float64 formula of tests/vectors.py::modulate cast to complex64
equals this for the (pi/2-)BPSK and QPSK schemes and differs by one ulp in places for 16/64/256-QAM
(tests/test_modulation_host.py pins that), so comparisons with the device are on bit patterns."""
import numpy as np

SCHEMES = (0, 1, 2, 4, 6, 8)  # modulation_scheme values: pi/2-BPSK, BPSK, QPSK, 16/64/256-QAM
SCALING_BITS = {0: 0x3F3504F3, 1: 0x3F3504F3, 2: 0x3F3504F3, 4: 0x3EA1E89B, 6: 0x3E1E01B3, 8: 0x3D9D130E}


def qm(mod: int) -> int:
    return 1 if mod in (0, 1) else mod


def scaling(mod: int) -> np.float32:
    return np.array([SCALING_BITS[mod]], np.uint32).view(np.float32)[0]


def _axis(s: np.ndarray) -> np.ndarray:
    """s_0 (2^(n-1) - s_1 (2^(n-2) - .. s_(n-1))) over the columns of s"""
    n = s.shape[1]
    t = s[:, n - 1].copy()
    for j in range(n - 2, -1, -1):
        t = s[:, j] * ((1 << (n - 1 - j)) - t)
    return t


def levels(bits: np.ndarray, mod: int) -> np.ndarray:
    """Unpacked bits -> int8 array (n, 2) of (re, im) levels."""
    q = qm(mod)
    s = 1 - 2 * np.asarray(bits, np.int32).reshape(-1, q)
    if q == 1:
        re, im = s[:, 0].copy(), s[:, 0]
        if mod == 0:
            re[1::2] = -re[1::2]
    else:
        re, im = _axis(s[:, 0::2]), _axis(s[:, 1::2])
    return np.stack([re, im], axis=1).astype(np.int8)


def modulate(bits: np.ndarray, mod: int) -> np.ndarray:
    """Unpacked bits -> complex64 symbols, float32(level) * scaling."""
    lv = levels(bits, mod).astype(np.float32) * scaling(mod)
    return np.ascontiguousarray(lv).view(np.complex64).reshape(-1)


def all_index_bits(mod: int) -> np.ndarray:
    """The bits of every symbol index in order (b0 the index's most significant bit); for the two BPSKs 0, 0, 1, 1 so
    that both symbol parities see both bits."""
    q = qm(mod)
    if q == 1:
        return np.array([0, 0, 1, 1], np.uint8)
    idx = np.arange(1 << q)
    return ((idx[:, None] >> np.arange(q - 1, -1, -1)) & 1).astype(np.uint8).reshape(-1)
