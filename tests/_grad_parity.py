"""Element-wise parity of per-parameter gradients (HIP step vs oracle).

A norm comparison is blind to errors that keep the norm: swapped kh / kw taps, flipped signs, permuted channels, a tile written to the
wrong place.  grad_parity checks every tensor element-wise (max-norm relative error), by direction (cosine) AND by norm."""
import torch

MAXNORM_TOL = 2e-3  # max |hip - ref| / max |ref| per tensor (the standard of tests/test_gpu_step.py::test_backward_vs_oracle)
COS_MIN = 0.99999


def norm_rel(hip, ref):
    """|‖hip‖ - ‖ref‖| / ‖ref‖ -- the norm-only check the element-wise one extends."""
    hn, rn = float(hip.double().norm()), float(ref.double().norm())
    return abs(hn - rn) / max(rn, 1e-300)


def tensor_parity(hip, ref):
    """(max-norm relative error, cosine, norm deviation) of one gradient tensor."""
    h, r = hip.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert h.shape == r.shape, (h.shape, r.shape)
    maxnorm = float((h - r).abs().max() / r.abs().max().clamp_min(1e-300))
    cos = float(torch.dot(h, r) / (h.norm() * r.norm()).clamp_min(1e-300))
    return maxnorm, cos, norm_rel(h, r)


def grad_parity(hip, ref, norm_tol, maxnorm_tol=MAXNORM_TOL, cos_min=COS_MIN, what=""):
    """hip / ref: {parameter name: gradient}.  Every parameter of `hip` must be in `ref`.  Per tensor: max-norm relative error <=
    maxnorm_tol, cosine >= cos_min, norm within norm_tol.  Returns the rows (name, maxnorm, cosine, norm dev); raises AssertionError
    naming every tensor that fails."""
    rows, bad = [], []
    missing = sorted(set(hip) - set(ref))
    assert not missing, f"{what}: gradients without a reference: {missing}"
    for k in hip:
        mn, cos, nr = tensor_parity(hip[k], ref[k])
        rows.append((k, mn, cos, nr))
        if not (mn <= maxnorm_tol and cos >= cos_min and nr <= norm_tol):
            bad.append((k, mn, cos, nr))
    if rows:
        w = max(rows, key=lambda t: t[1])
        print(f"{what}: {len(rows)} gradient tensors, worst max-norm rel {w[0]} {w[1]:.2e}, "
              f"min cosine {min(t[2] for t in rows):.7f}, worst norm dev {max(t[3] for t in rows):.2e}")
    assert not bad, f"{what}: gradient parity violated (name, max-norm rel, cosine, norm dev): {bad}"
    return rows
