"""An independent restatement of the two curves fadtk_amd.mauve draws from a pair of cell histograms (test plumbing, not product):
the divergence frontier of MAUVE (Pillutla et al. 2021) with its area, and the PRD curve of Sajjadi et al. 2018 with its two F-values.
Plain Python loops over the cells in float64 and a trapezoid rule of its own -- nothing shared with the module under test."""
import math

import numpy as np


def kl(a, b):
    total = 0.0
    for ai, bi in zip(a, b):
        if ai > 0:
            total += ai * math.log(ai / bi)
    return total


def frontier(p, q, scale=5.0, points=25):
    """-> list of (x, y): (exp(-s KL(q || r)), exp(-s KL(p || r))), r = lam p + (1 - lam) q, plus (0, 1) and (1, 0)"""
    out = []
    for i in range(points):
        lam = 1e-6 + (1 - 2e-6) * i / (points - 1)
        r = [lam * pi + (1 - lam) * qi for pi, qi in zip(p, q)]
        out.append((math.exp(-scale * kl(q, r)), math.exp(-scale * kl(p, r))))
    return out + [(0.0, 1.0), (1.0, 0.0)]


def _trapezoid(xs, ys):
    pts = sorted(zip(xs, ys))
    return sum(0.5 * (x1 - x0) * (y0 + y1) for (x0, y0), (x1, y1) in zip(pts[:-1], pts[1:]))


def mauve(p, q, scale=5.0, points=25):
    pts = frontier(p, q, scale, points)
    xs, ys = [a for a, _ in pts], [b for _, b in pts]
    return max(_trapezoid(xs, ys), _trapezoid(ys, xs))


def prd(p, q, angles=1001):
    """-> (precision list, recall list)"""
    precision, recall = [], []
    for i in range(angles):
        theta = 1e-10 + (math.pi / 2 - 2e-10) * i / (angles - 1)
        lam = math.tan(theta)
        a = sum(min(lam * pi, qi) for pi, qi in zip(p, q))
        precision.append(a)
        recall.append(a / lam)
    return precision, recall


def f_beta(precision, recall, beta):
    return max((1 + beta * beta) * a * b / (beta * beta * a + b + 1e-10) for a, b in zip(precision, recall))


def metrics(p_counts, q_counts, scale=5.0, points=25):
    p = [c / float(sum(p_counts)) for c in p_counts]
    q = [c / float(sum(q_counts)) for c in q_counts]
    precision, recall = prd(p, q)
    return {"mauve": mauve(p, q, scale, points), "f_beta": f_beta(precision, recall, 8.0), "f_beta_inv": f_beta(precision, recall, 0.125),
            "prd_precision": np.array(precision), "prd_recall": np.array(recall), "divergence_curve": np.array(frontier(p, q, scale, points))}
