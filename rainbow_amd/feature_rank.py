"""The spectrum of a feature matrix from its sample-side Gram matrix: srank (Kumar, Agarwal, Ghosh, Levine, "Implicit
Under-Parameterization Inhibits Data-Efficient Deep RL", ICLR 2021), the feature rank of Lyle, Rowland, Dabney ("Understanding and
Preventing Capacity Loss in RL", ICLR 2022) and the effective rank of Roy & Vetterli (2007).  Host side, numpy only: the Gram
matrix K = Phi Phi^T comes from the device (rb_gram_f64, csrc/feature_gram.h), a small [n, n] float64 matrix; the eigenvalues are
LAPACK's.  Nothing here touches the GPU."""
import numpy as np

_NAN = float("nan")


def spectrum_metrics(K, n, d, eps=0.01, delta=0.01):
    """K: float64 [n, n], the Gram matrix Phi Phi^T of n feature rows of dimension d (uncentred).

    lambda = eigvalsh(K / n); sigma_i = sqrt(max(lambda_i, 0)) in descending order, the first min(n, d) of them: the singular values
    of Phi / sqrt(n) (the rest are zero in exact arithmetic).  Returns a dict:
      singular_values   float64 [min(n, d)], descending
      feature_rank      #{sigma_i > eps}                                           (Lyle et al.: singular values of Phi / sqrt(n))
      srank             min k with sum_{i <= k} sigma_i / sum_i sigma_i >= 1 - delta   (Kumar et al.); 0 when every sigma is 0
      effective_rank    exp(-sum p_i ln p_i), p_i = sigma_i / sum sigma, over p_i > 0; 0.0 when every sigma is 0
      mean_sq_norm      trace(K) / n, the mean squared feature norm
      top_share         sigma_1^2 / sum sigma_i^2 (NaN when every sigma is 0)
      finite            False when K holds a NaN or an inf: checked BEFORE LAPACK sees it; the metrics are then NaN (the ranks too,
                        as floats) and singular_values is all NaN — no exception.

    Resolution floor: K accumulated in double carries an error of about d 2^-53 sigma_1^2 n per entry bound, which moves the
    eigenvalues of K / n by up to about d 2^-53 sigma_1^2: a sigma below sigma_1 sqrt(d 2^-53) is noise (2e-7 sigma_1 at d = 512,
    6e-7 sigma_1 at d = 3136).  Keep eps well above that floor; the default 0.01 is."""
    n, d = int(n), int(d)
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (n, n):
        raise ValueError("spectrum_metrics: K must be [%d, %d], got %r" % (n, n, K.shape))
    r = min(n, d)
    if not np.isfinite(K).all():
        return {"singular_values": np.full(r, np.nan), "feature_rank": _NAN, "srank": _NAN, "effective_rank": _NAN,
                "mean_sq_norm": _NAN, "top_share": _NAN, "finite": False}
    lam = np.linalg.eigvalsh(K / float(n))
    sigma = np.sqrt(np.maximum(lam[::-1][:r], 0.0))
    total = float(sigma.sum())
    out = {"singular_values": sigma, "feature_rank": int((sigma > eps).sum()), "mean_sq_norm": float(np.trace(K)) / n, "finite": True}
    if total > 0.0:
        share = np.cumsum(sigma) / total
        out["srank"] = int(min(r, np.searchsorted(share, 1.0 - delta, side="left") + 1))
        p = sigma[sigma > 0.0] / total
        out["effective_rank"] = float(np.exp(-(p * np.log(p)).sum()))
        out["top_share"] = float(sigma[0] ** 2 / (sigma ** 2).sum())
    else:
        out.update(srank=0, effective_rank=0.0, top_share=_NAN)
    return out
