"""The inputs of test_gpu_running_sums.py judged on the CPU: numpy's mean IS the float32 running sum the reference writes out, and the
hostile rows tell that sum from every wrong order tried -- which the older Gaussian cases cannot."""
import numpy as np
import pytest

import running_sum_reference as RS


def _premise_cases():
    seen = []
    for _, dtype, d, n, _ in RS.PLAIN_CASES:
        if dtype != "bfloat16" and (dtype, d, n) not in seen:
            seen.append((dtype, d, n))
    return seen


def test_numpys_mean_is_the_sequential_float32_sum():
    """np.mean(x, axis=0) of float16 and float32 rows = the float32 sum of the rows one after the other, divided in float64 and cast
    back, at every (dtype, d, n) of the plain-update table: the reference of the GPU test is numpy's own mean."""
    cases = _premise_cases()
    assert len(cases) > 50                              # (never an empty loop)
    for dtype, d, n in cases:
        x = RS.rows_for(dtype, d, n)
        got = RS.mean_of(RS.running_sum(RS.as_f32(x)), n).astype(x.dtype)
        want = np.mean(x, axis=0)
        assert want.dtype == x.dtype
        np.testing.assert_array_equal(got, want, err_msg=f"{dtype} d={d} n={n}")


def test_hostile_rows_tell_the_sequential_sum_from_every_wrong_order():
    """For every matrix the GPU test walks, of 33 rows or more: groups of 4, groups of 16, two merged halves and the exact sum rounded
    once each change the float32 mean in at least 25 % of its columns, one row too many in at least 50 % (half the worst shares seen at
    d = 64 when the rows were designed).  A walk with such an error fails the GPU test in those columns."""
    short, lowest, first = [], {}, {}
    count = 0
    for label, x in RS.order_inputs():
        n = x.shape[0]
        if n < RS.SHARP_FROM:
            continue
        count += 1
        sh = RS.shares(x)
        for name, _, bound in RS.WRONG_ORDERS:
            if not sh[name] >= bound:
                short.append((label, name, sh[name], bound))
            lowest[name] = min(lowest.get(name, 1.0), sh[name])
        key = label.split(" n=")[0].split(" length=")[0]
        first.setdefault(key, n)
        first[key] = min(first[key], n)
    assert count > 100
    print("\nlowest share of columns changed, per wrong order: " + ", ".join(f"{k} {v:.2f}" for k, v in lowest.items()))
    print("smallest row count held to the shares, per kind of input: " + ", ".join(f"{k}: {v}" for k, v in sorted(first.items())))
    assert not short, short[:20]


@pytest.mark.parametrize("n,d,offset", [(513, 512, 10.0)])
def test_the_older_gaussian_case_cannot_see_the_order(n, d, offset):
    """Why the hostile rows exist.  The rows of test_calc_embd_statistics_returns_numpys_own_mean_for_frames_with_an_offset at
    (513, 512, 10.0) are float16 values at one scale: their float32 sum is exact, so the sequential sum and the exact sum rounded once
    agree in EVERY column -- a walk that regrouped the rows, merged partial sums or returned the exact sum passes that case."""
    x = RS.as_f32(RS.gaussian_rows(n, d, offset, np.float16))
    np.testing.assert_array_equal(RS.running_sum(x), RS.exact_rounded(x))
    np.testing.assert_array_equal(RS.running_sum(x), RS.grouped(x, 16))
