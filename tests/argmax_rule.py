"""The argmax clause on the rows the parity tests exclude as not clear (reference top-2 gap <= 1e-9): there the two
argmaxes may differ, but the reference's argmax must still be a near-maximum of the device's own row."""
import numpy as np

CLEAR_GAP = 1e-9          # the project's clear-gap rule


def assert_unclear_rows_near_max(p_hip, argmax_ref, clear, drift, what):
    """For every row that is not clear: p_hip[n, argmax_ref[n]] >= p_hip[n].max() - margin, with margin = the clear-gap
    rule plus six times `drift`, the largest element-wise relative deviation of theta, eta and p from the reference
    that the calling test measured (three factors, both rows of the comparison, entries of P at most 1).  Prints and
    returns (rows not clear, rows whose argmax differs, largest gap among them)."""
    rows = np.flatnonzero(~np.asarray(clear, dtype=bool))
    margin = CLEAR_GAP + 6.0 * float(drift)
    ref = np.asarray(argmax_ref)[rows].astype(np.int64)
    gap = p_hip[rows].max(axis=1) - p_hip[rows, ref] if len(rows) else np.zeros(0)
    differ = int((np.argmax(p_hip[rows], axis=1) != ref).sum()) if len(rows) else 0
    worst = float(gap.max()) if len(rows) else 0.0
    print(f"{what}: {len(rows)} of {len(clear)} rows not clear, {differ} with another argmax than the reference's, "
          f"largest gap to the device's own maximum {worst:.3e} (margin {margin:.3e})")
    assert worst <= margin, f"{what}: reference argmax {worst:.3e} below the device row's maximum (margin {margin:.3e})"
    return len(rows), differ, worst
