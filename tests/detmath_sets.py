"""The argument sets of the deterministic logarithm and exponential (oracle/detmath.h; det_logf / det_expf of azh_device.h),
shared by the CPU accuracy test (tests/test_detmath_accuracy.py) and the device's bit-for-bit test
(tests/test_gpu_detmath_edges.py).  Every set is a sorted float32 array (a "run": the function is to be non-decreasing along
it), at most 2^24 long.

(-2^-20, 2^-20) holds 1.8e9 floats, more than a test of seconds can visit: there exp(x) rounds to one of 1 - 2^-24, 1 and
1 + 2^-23 .. , so the set takes 2^10 mantissas of every binade of both signs (the denormal one included), every float within
2^12 steps of zero and of +-2^-20, and +-0."""
import numpy as np

U32, F32 = np.uint32, np.float32
LOGF_WORST = 0x3FB4F239     # 0.827 ulp, the worst of all positive normal floats
EXPF_WORST = 0xC0BC17A1     # 1.010 ulp, the worst of all floats in [-87, 88]
FLT_MIN_BITS, FLT_MAX_BITS = 0x00800000, 0x7F7FFFFF


def bits(b):
    return np.asarray(b, dtype=U32).view(F32)


def _binade(e, step=1):
    """the positive floats of biased exponent e, every `step`-th mantissa"""
    return bits((U32(e) << U32(23)) | np.arange(0, 1 << 23, step, dtype=U32))


def _between(lo, hi):
    """every float in [lo, hi], both of one sign and non-zero, ascending"""
    a, b = int(F32(lo).view(U32)), int(F32(hi).view(U32))
    if lo < 0:
        return bits(np.arange(a, b - 1, -1, dtype=np.int64).astype(U32))
    return bits(np.arange(a, b + 1, dtype=np.int64).astype(U32))


def logf_runs():
    """{name: sorted run} of positive normal arguments"""
    others = np.concatenate([_binade(e, 1 << 13) for e in range(1, 255) if e not in (126, 127)])
    return {"[0.5, 2)": np.concatenate([_binade(126), _binade(127)]),
            "other binades": np.sort(others),
            "worst": bits([LOGF_WORST - 1, LOGF_WORST, LOGF_WORST + 1])}


def logf_near_one():
    """every float in [1 - 2^-10, 1 + 2^-10]"""
    return _between(1.0 - 2.0 ** -10, 1.0 + 2.0 ** -10)


def gumbel_grid():
    """u = (i + 0.5) * 2^-23, i < 2^23: every argument gumbel_noise passes to the outer det_logf (exact in f32)"""
    u = ((np.arange(1 << 23, dtype=np.float32) + F32(0.5)) * F32(2.0 ** -23)).astype(F32)
    assert u[0] > 0 and u[-1] < 1 and (np.diff(u) > 0).all()
    return u


def expf_runs():
    """{name: sorted run}; the runs inside [-87, 88] are the ones an error bound applies to"""
    tiny_pos = np.concatenate([_binade(e, 1 << 13) for e in range(0, 107)] +
                              [bits(np.arange(0, 1 << 12, dtype=U32)), _between(2.0 ** -20 * (1 - 2.0 ** -12), 2.0 ** -20)[:-1]])
    tiny_pos = np.unique(tiny_pos)                       # (sorted; +0 first)
    tiny = np.concatenate([-tiny_pos[::-1], tiny_pos])   # ... -0, +0 ...
    lo, hi = _between(-87.0, -(2.0 ** -20)), _between(2.0 ** -20, 88.0)
    rest = np.concatenate([lo[::max(1, len(lo) // (1 << 21))], hi[::max(1, len(hi) // (1 << 21))]])
    return {"[-87.5, -86.5]": _between(-87.5, -86.5), "[87.5, 88.5]": _between(87.5, 88.5), "(-2^-20, 2^-20)": tiny,
            "rest": rest, "worst": bits([EXPF_WORST + 1, EXPF_WORST, EXPF_WORST - 1])}


def specials():
    """what no sweep holds: NaNs quiet and signalling of both signs, infinities, zeros, the denormal range's ends, FLT_MIN and
    its predecessor, FLT_MAX, the exponential's cut-offs with their neighbours, negative arguments"""
    m87, p88 = int(F32(-87.0).view(U32)), int(F32(88.0).view(U32))
    b = [0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC00001, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,
         0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
         FLT_MIN_BITS, FLT_MIN_BITS - 1, FLT_MIN_BITS + 1, 0x80800000, FLT_MAX_BITS, 0xFF7FFFFF,
         m87 - 2, m87 - 1, m87, m87 + 1, m87 + 2, p88 - 2, p88 - 1, p88, p88 + 1, p88 + 2,
         int(F32(-1.0).view(U32)), int(F32(-0.5).view(U32)), int(F32(-2.5).view(U32)), int(F32(-1e30).view(U32)),
         int(F32(1.0).view(U32)), int(F32(-87.33654475).view(U32))]
    return bits(b)


def ulp_error(got, ref):
    """|got - ref| in units of the f32 spacing just above |ref| (ref float64, non-zero and normal in f32)"""
    _, e = np.frexp(np.abs(ref))
    return np.abs(got.astype(np.float64) - ref) / np.ldexp(1.0, e - 24)


LOGF_ULP, EXPF_ULP = 0.85, 1.05
