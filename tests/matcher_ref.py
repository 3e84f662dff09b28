"""The float32 primitives the scalar referees of the ORBmatcher family share (tests only): fuse_ref,
triangulation_ref, point_refresh_ref, bow_common and test_oracle_match restate the reference's loops on top of
these, so that bit-exactness is decided by one model of each operation.

What is deliberately not here: cv::norm and the camera centre.  point_refresh_ref and triangulation_ref each keep
their own, with their reading in the docstring.
"""
import math
from fractions import Fraction

import numpy as np

HISTO = 30                       # ORBmatcher::HISTO_LENGTH


def f32(x):
    return np.float32(x)


def round_f32(fr):
    """A rational rounded to the nearest float, ties to even (subnormals included)."""
    if fr == 0:
        return f32(0.0)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                                      # 2^e <= a < 2^(e+1)
    q = max(e - 23, -149)
    n = a / Fraction(2) ** q
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    return f32(math.copysign(math.ldexp(fl, q), fr))                # exact in double (fl <= 2^24), inf on overflow


def fma(a, b, c):
    """fmaf(a, b, c): the exact a*b + c rounded once."""
    a, b, c = float(f32(a)), float(f32(b)), float(f32(c))
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return f32(np.float64(a) * np.float64(b) + np.float64(c))  # inf / NaN propagate as in fmaf
    return round_f32(Fraction(a) * Fraction(b) + Fraction(c))


def mat3(T, x, c=None, transpose=False, sign=1.0):
    """cv::Mat 3x3 * 3x1 (+ 3x1): each row summed in double, rounded once (the matcher family's reading)."""
    T = np.asarray(T, np.float32).reshape(4, 4)
    out = []
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(T[k, r] if transpose else T[r, k]) * float(x[k])
        s *= sign
        if c is not None:
            s += float(c[r])
        out.append(f32(s))
    return out


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance (:1647-1662): the popcount of the XOR."""
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def rotation_bin(a1, a2):
    """The rotation-histogram bin of two keypoint angles: round((a1 - a2 [+ 360]) * (1.0f / HISTO_LENGTH)), bin
    HISTO_LENGTH wrapped to 0 (factor :172, the bin :263-266)."""
    rot = f32(a1) - f32(a2)
    if rot < 0:
        rot = rot + f32(360.0)
    x = rot * f32(1.0 / HISTO)
    bn = int(np.floor(abs(float(x)) + 0.5)) * (1 if x >= 0 else -1)   # roundf
    return 0 if bn == HISTO else bn


def three_maxima(counts):
    """ORBmatcher::ComputeThreeMaxima (:1601-1645) on the bin sizes: the three indices, -1 for a dropped one."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(counts):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if m2 < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif m3 < f32(0.1) * f32(m1):
        i3 = -1
    return i1, i2, i3
