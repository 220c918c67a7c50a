"""Detection events in float64, the way the reference runs (utils/evaluate_models.py:185-218): ``np.convolve(..., 'same')`` of each
segment with ``ones(win) / win``, then the ``prev_wake`` walk of :206-216 over the smoothed values - extended to record where a run
starts, where it ends and where it is greatest, instead of only counting its first row.  NumPy only; the yardstick of
tests/test_gpu_events.py (e) and the statement tests/test_events_host.py pins on hand-written cases.

``np.convolve`` sums its products in another order than the library's ascending chain, so its values differ from the library's in the
last bits: comparisons against this file need a margin around the threshold (``margin``) and between a run's two greatest values
(``peak_gap``)."""
import numpy as np


def smooth(p, win):
    """``np.convolve(p, ones(win) / win, 'same')`` in float64 for a segment of at least ``win`` rows; for a shorter one - where 'same'
    would return ``win`` values - the same centre of the full convolution, ``full[(win - 1) // 2:][:len(p)]``.  ``win <= 0``: ``p``."""
    p = np.asarray(p, np.float64)
    if win <= 0 or p.size == 0:
        return p.copy()
    k = np.ones((win,)) / win
    if p.size >= win:
        return np.convolve(p, k, mode="same")
    return np.convolve(p, k, mode="full")[(win - 1) // 2:][:p.size]


def walk(sm, threshold):
    """The reference's loop over one smoothed segment: ``[(start, end, peak, peak_value)]``, one entry where the reference counts one
    false alarm.  ``peak`` is the first row of the run at which ``sm`` is greatest."""
    out = []
    prev_wake = False
    for i, posterior in enumerate(sm):
        if posterior > threshold and not prev_wake:
            out.append([i, i + 1, i, float(posterior)])      # the reference's `accepts += 1`
        elif posterior > threshold:
            out[-1][1] = i + 1
            if posterior > out[-1][3]:
                out[-1][2], out[-1][3] = i, float(posterior)
        prev_wake = False
        if posterior > threshold:
            prev_wake = True
    return [tuple(e) for e in out]


def events(post, thresholds, seg_offs=None, win=30):
    """``post`` 1-D or ``[planes, n]``; one threshold per plane.  Returns ``(events, smoothed)``: the events as tuples ``(plane, seg,
    start, end, peak, peak_value)`` in plane, segment, start order, and per plane the list of the segments' smoothed values."""
    post = np.asarray(post, np.float32)
    if post.ndim == 1:
        post = post[None]
    thr = np.broadcast_to(np.asarray(thresholds, np.float64), (post.shape[0],))
    offs = np.array([0, post.shape[1]], np.int64) if seg_offs is None else np.asarray(seg_offs, np.int64)
    ev, sms = [], []
    for k in range(post.shape[0]):
        sms.append([])
        for u in range(len(offs) - 1):
            sm = smooth(post[k, offs[u]:offs[u + 1]], win)
            sms[-1].append(sm)
            ev += [(k, u) + e for e in walk(sm, thr[k])]
    return ev, sms


def margin(sms, thresholds):
    """The smallest ``|sm - threshold|`` over all planes and segments (inf where there are no rows)."""
    thr = np.broadcast_to(np.asarray(thresholds, np.float64), (len(sms),))
    d = [np.abs(sm - thr[k]).min() for k, segs in enumerate(sms) for sm in segs if sm.size]
    return min(d) if d else np.inf


def peak_gap(sms, event):
    """The difference between the two greatest smoothed values of an event's run (inf for a run of one row)."""
    k, u, a, b = event[:4]
    v = np.sort(sms[k][u][a:b])
    return v[-1] - v[-2] if v.size > 1 else np.inf
