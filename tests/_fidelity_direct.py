"""SSIM of one 8 x 8 window the direct way: float64 means, population variances and covariance over the 64 samples, C1 = (0.01 * 255)^2 = 6.5025 and
C2 = (0.03 * 255)^2 = 58.5225.  What tests/_fidelity_ref.py's integer form is a restatement of (everything scaled by 64^2, the constants rounded)."""
import numpy as np

C1, C2 = 6.5025, 58.5225


def ssim_window(ga, gb):
    ga, gb = np.asarray(ga, np.float64), np.asarray(gb, np.float64)
    assert ga.shape == gb.shape == (8, 8)
    m1, m2 = ga.mean(), gb.mean()
    v1, v2 = ((ga - m1) ** 2).mean(), ((gb - m2) ** 2).mean()
    cov = ((ga - m1) * (gb - m2)).mean()
    return ((2.0 * m1 * m2 + C1) * (2.0 * cov + C2)) / ((m1 * m1 + m2 * m2 + C1) * (v1 + v2 + C2))
