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
# the standard rates of include/wwhip.h ("every pair ... passes"), and their 132 ordered pairs
STANDARD = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)
PAIRS = tuple((a, b) for a in STANDARD for b in STANDARD if a != b)
# One or two pairs of every class the tile planner distinguishes (`plan_class` below), and the extremes of up, down and the table:
#   decim, 63 / 100 / 136 / 209 lanes and 256 lanes with ne8 = 128 | phase with ne8 = 0 | 64 | 128 | 256 and a large up
CLASS_REPS = ((192000, 8000), (176400, 11025), (192000, 16000), (192000, 24000), (96000, 16000),
              (192000, 11025), (32000, 11025), (176400, 8000),
              (176400, 16000),
              (88200, 16000), (48000, 11025),
              (11025, 192000), (8000, 192000), (16000, 48000), (16000, 44100), (500000, 16000))
ZEROS, ROLLOFF, BETA = 32, 0.945, 14.769656459379492


def design(rate_in, rate_out=16000, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    r = Fraction(rate_out, rate_in)
    up, down = r.numerator, r.denominator
    L = rate_in * up
    f2 = rolloff * min(rate_in, rate_out) / L
    half = int(ceil(zeros / f2))
    win = np.kaiser(2 * half + 1, beta)
    i = np.arange(-half, half + 1)
    h = up * f2 * np.sinc(f2 * i) * win[i + half]
    return up, down, half, h.astype(np.float64)


def tpp(up, half):
    return (2 * half + 1 + up - 1) // up


XCAP, R8, R1 = 12288, 8, 7   # floats a tile stages; outputs per item of the long phase form; outputs per lane of the up == 1 form


def plan_class(up, down, half):
    """The tile geometry the library derives for a filter, restated: (form, ne8, ne1, lanes1).  'decim' (up == 1): a tile is lanes1
    lanes of R1 outputs, lanes1 = as many as fit the staged span.  'phase': a tile is ne8 items of R8 outputs for long ranges
    (ne8 = the largest of 256, 128, 64 whose worst-case span fits, else 0) and ne1 items of one output for short ones."""
    t = tpp(up, half)

    def span(R, ne):
        return ((ne - 1) // up + 2) * R * down + t + 2

    ne8 = next((ne for ne in (256, 128, 64) if span(R8, ne) <= XCAP), 0)
    ne1 = next((ne for ne in (256, 128, 64, 32, 16, 8, 4, 2, 1) if span(1, ne) <= XCAP), 0)
    lanes1 = 0
    if up == 1:
        n_u = -(-((R1 - 1) * down + 2 * half + 1) // 4) * 4
        if n_u <= XCAP:
            lanes1 = min(256, (XCAP - n_u) // (R1 * down) + 1)
    return ("decim" if lanes1 else "phase"), ne8, ne1, lanes1


def tile_outputs(up, down, half, count):
    """Outputs per tile of the form a range of `count` outputs takes."""
    form, ne8, ne1, lanes1 = plan_class(up, down, half)
    return lanes1 * R1 if form == "decim" else ne8 * R8 if ne8 and count >= 2 * R8 * up else ne1


def out_len(n, up, down):
    return (n * up + down - 1) // down


def direct(x, up, down, half, h, in_first=0, out_first=0, count=None):
    """Outputs [out_first, out_first + count) of the signal whose samples in_first .. in_first + len(x) - 1 are x (zero elsewhere)."""
    x = np.asarray(x, np.float64)
    if count is None:
        count = out_len(in_first + len(x), up, down) - out_first
    y = np.zeros(count, np.float64)
    T = 2 * half // up + 2
    rows = max(64, 2 ** 22 // T)                               # the [rows, T] temporaries stay at some tens of megabytes
    for a in range(0, count, rows):
        m = out_first + np.arange(a, min(a + rows, count), dtype=np.int64)
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
