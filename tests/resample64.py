"""Float64 reference of the polyphase resampler (wwhip/resample.py, csrc/resample.hip): its own statement of the filter and of
y[m], sharing no code with the package.

    g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g, L = rate_in * up
    f2 = rolloff * min(rate_in, rate_out) / L, half = ceil(zeros / f2)
    h[i] = up * f2 * sinc(f2 i) * kaiser(2 half + 1, beta)[i + half]
    y[m] = sum_k h[m down - k up] x[k],  |m down - k up| <= half,  x = 0 outside the clip,  m < ceil(n up / down)

`direct` evaluates the sum as written (any output range of a signal given in part: what a stream's packets need); `poly` is
scipy.signal.resample_poly(x, up, down, window=h / up), for long inputs.  `bound_sum` is A[m] = sum |h| |x| by the same routines.
"""
from fractions import Fraction
from math import ceil

import numpy as np

RATES = (48000, 44100, 32000, 24000, 22050, 11025, 8000)
ZEROS, ROLLOFF, BETA = 32, 0.945, 14.769656459379492


def design(rate_in, rate_out=16000, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    r = Fraction(rate_out, rate_in)
    up, down = r.numerator, r.denominator
    L = rate_in * up
    f2 = rolloff * min(rate_in, rate_out) / L
    half = int(ceil(zeros / f2))
    win = np.kaiser(2 * half + 1, beta)
    h = np.array([up * f2 * np.sinc(f2 * i) * win[i + half] for i in range(-half, half + 1)], np.float64)
    return up, down, half, h


def tpp(up, half):
    return (2 * half + 1 + up - 1) // up


def out_len(n, up, down):
    return (n * up + down - 1) // down


def direct(x, up, down, half, h, in_first=0, out_first=0, count=None):
    """Outputs [out_first, out_first + count) of the signal whose samples in_first .. in_first + len(x) - 1 are x (zero elsewhere)."""
    x = np.asarray(x, np.float64)
    if count is None:
        count = out_len(in_first + len(x), up, down) - out_first
    y = np.zeros(count, np.float64)
    T = 2 * half // up + 2
    for a in range(0, count, 4096):
        m = out_first + np.arange(a, min(a + 4096, count), dtype=np.int64)
        kmin = -((half - m * down) // up)                      # ceil((m down - half) / up)
        k = kmin[:, None] + np.arange(T, dtype=np.int64)[None, :]
        i = m[:, None] * down - k * up                         # descending from <= half
        j = k - in_first
        ok = (i >= -half) & (j >= 0) & (j < len(x))
        hv = h[np.where(ok, i + half, 0)]
        xv = x[np.where(ok, j, 0)] if len(x) else np.zeros_like(hv)
        y[a:a + len(m)] = np.where(ok, hv * xv, 0.0).sum(axis=1)
    return y


def poly(x, up, down, h):
    from scipy.signal import resample_poly
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return np.zeros(0, np.float64)
    return resample_poly(x, up, down, window=h / up)[:out_len(len(x), up, down)]


def resample(x, rate_in, rate_out=16000):
    """The reference output of a whole clip (int16 is scaled by 1 / 32768 first)."""
    x = np.asarray(x)
    x = x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)
    if rate_in == rate_out:
        return x
    up, down, half, h = design(rate_in, rate_out)
    return direct(x, up, down, half, h) if len(x) <= 4096 else poly(x, up, down, h)


def bound_sum(x, rate_in, rate_out=16000):
    """A[m] = sum_k |h[m down - k up]| |x[k]|."""
    x = np.asarray(x)
    x = np.abs(x.astype(np.float64)) / 32768.0 if x.dtype == np.int16 else np.abs(x.astype(np.float64))
    if rate_in == rate_out:
        return x
    up, down, half, h = design(rate_in, rate_out)
    return direct(x, up, down, half, np.abs(h)) if len(x) <= 4096 else poly(x, up, down, np.abs(h))


def tones(rate, n, f_nyq):
    """The tone-test signal sampled at `rate`: 97, 440, 1234.5, 0.4 f_N, 0.7 f_N Hz with amplitudes 0.2, 0.2, 0.2, 0.1, 0.1."""
    t = np.arange(n, dtype=np.float64) / rate
    return sum(a * np.sin(2 * np.pi * f * t) for f, a in ((97.0, 0.2), (440.0, 0.2), (1234.5, 0.2), (0.4 * f_nyq, 0.1), (0.7 * f_nyq, 0.1)))
