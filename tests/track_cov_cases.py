"""What tests/test_track_cov_cpu.py and tests/test_track_cov_gpu.py share: generated pose-point records, the documented edge cases, and the
checks of a returned covariance against numpy (the bounds are derived in test_track_cov_cpu.py's docstring)."""
import numpy as np

EPS = 2.0 ** -52


def make_records(n, ncam, seed, found_frac=0.8, zero_w_frac=0.15):
    """n records of ncam cameras in front of a rig: world points 2-6 units ahead, camera derivatives of a 100-pixel focal length, level noise
    1, 1/2, 1/4, 1/8, a mix of found / not found and of zero weights.  Returns (records, weights, CamFromBase (R, t) list, refined (R, t),
    mu_last)."""
    from mcptam_amd.keyframe import POSE_POINT_DTYPE
    from mcptam_amd.pvs import se3_exp, so3_exp
    rng = np.random.default_rng(seed)
    cfbs = [(np.eye(3), np.zeros(3))] + [(so3_exp(rng.normal(0, 0.2, 3)), rng.normal(0, 0.05, 3)) for _ in range(ncam - 1)]
    refined = se3_exp(rng.normal(0, 0.05, 6))
    mu = rng.normal(0, 2e-3, 6)
    p = np.zeros(n, dtype=POSE_POINT_DTYPE)
    p["world_pos"] = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 6.0, n)], axis=1)
    p["cam_derivs"] = rng.normal(0, 30.0, (n, 4)) + np.array([100.0, 0.0, 0.0, 100.0])
    p["sqrt_inv_noise"] = 0.5 ** rng.integers(0, 4, n)
    p["cam"] = rng.integers(0, ncam, n)
    p["found"] = rng.random(n) < found_frac
    p["found_pos"] = rng.uniform(0, 640, (n, 2)); p["image"] = p["found_pos"] + rng.normal(0, 1, (n, 2))
    w = rng.uniform(0.05, 1.0, n)
    w[rng.random(n) < zero_w_frac] = 0.0
    return p, w, cfbs, refined, mu


def check_against_numpy(rec, tag=""):
    """The returned cov against numpy's truncated pseudo-inverse of the RETURNED info, the module's bounds.  Returns the two measured
    figures in units of kappa 2^-52."""
    from mcptam_amd.pvs import pinv_truncated, pose_cov_arrays
    info, cov, eig = pose_cov_arrays(rec)
    assert np.array_equal(info, info.T) and np.array_equal(cov, cov.T)
    assert np.all(np.diff(eig) <= 0)
    kappa = float(np.linalg.cond(info))
    assert kappa <= 1e6, kappa
    want, lam, rank = pinv_truncated(info)
    assert rank == 6 and rec.rank == 6
    d = np.linalg.norm(cov - want) / np.linalg.norm(cov)
    r = np.abs(cov @ info - np.eye(6)).max()
    print(tag, "kappa %.3g  |cov - pinv|_F / |cov|_F = %.3g (%.3g kappa eps)  |cov info - I|_max = %.3g (%.3g kappa eps)  sweeps %d" %
          (kappa, d, d / (kappa * EPS), r, r / (kappa * EPS), rec.sweeps))
    assert d <= 64 * kappa * EPS and r <= 64 * kappa * EPS
    assert np.abs(eig - lam).max() <= 64 * EPS * lam[0]                 # (eigenvalues of a symmetric matrix: absolute error of order eps |A|)
    assert abs(rec.norm_fro - np.linalg.norm(cov)) <= 32 * EPS * rec.norm_fro          # (36 positive terms on either side: under 20 x 2^-53 each)
    assert 0 <= rec.sweeps <= 16
    return d / (kappa * EPS), r / (kappa * EPS)


def rank2_case():
    pts, w, cfbs, refined, mu = make_records(1, 1, 11)
    pts["found"] = 1; pts["sqrt_inv_noise"] = 1e6; w[:] = 1.0
    return pts, w, cfbs, refined, mu


def check_rank2(rec):
    """One record with sqrt_inv_noise = 1e6: two eigenvalues of order 1e15, the four of the prior (100) fall under lambda_max / 1e9 and are
    truncated.  cov against numpy's truncated pseudo-inverse of the returned info: the bound of the module with kappa the condition number
    of the part that is kept."""
    from mcptam_amd.pvs import pinv_truncated, pose_cov_arrays
    info, cov, eig = pose_cov_arrays(rec)
    want, lam, rank = pinv_truncated(info)
    assert rec.valid == 1 and rec.n_used == 1 and rank == 2 and rec.rank == 2
    assert np.all(eig[2:] * 1e9 <= eig[0]) and np.all(eig[:2] * 1e9 > eig[0])
    kappa = lam[0] / lam[1]
    d = np.linalg.norm(cov - want) / np.linalg.norm(cov)
    print("rank 2: eig", eig.tolist(), "kappa kept %.3g  |cov - pinv|_F / |cov|_F = %.3g" % (kappa, d))
    assert d <= 64 * kappa * EPS
    assert np.array_equal(cov, cov.T) and np.linalg.matrix_rank(cov, tol=1e-6 * np.abs(cov).max()) == 2


def nan_case():
    pts, w, cfbs, refined, mu = make_records(70, 2, 13)
    pts["found"] = 1; w[:] = 0.5
    pts["cam_derivs"][66, 2] = np.nan
    return pts, w, cfbs, refined, mu


def check_nan(rec):
    from mcptam_amd.pvs import pose_cov_arrays
    info, cov, eig = pose_cov_arrays(rec)
    assert rec.valid == -1 and rec.n_used == 70 and rec.rank == 0 and rec.sweeps == 0
    assert np.isnan(info).any() and not cov.any() and not eig.any() and rec.norm_fro == 0.0
