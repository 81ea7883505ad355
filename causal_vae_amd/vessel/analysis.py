"""What the reference does with a trained CausalVesselVAE (vessel_analysis/03_evaluate_vessel, 04_generate_counterfactual), as batched calls.

Every consumer there runs the decoder half in eval mode, one small batch at a time.  Here each one is a few large decodes through
CausalVesselVAE.encode / .decode (eval mode: BatchNorm folded into the convs) and one reduction kernel (csrc/vessel_infer.hip):
  feature_importance ...... analyze_vessel.py:68-121          (cvae_row_diff_norms)
  ensemble_reconstruction . ensemble_reconstruction.py:57-89  (cvae_stack_mean_std)
  z_permutation_grid ...... check_mechanism_z_perm.py:100-130
All three are inference only (no_grad) and expect the models in eval mode, as the reference puts them.
"""
import torch

from .. import ops

DEFAULT_CHUNK_ROWS = 64        # decoded rows per call: the 31 MB-per-row fp32 intermediate (384 x 640 x 32) of 64 rows is 2 GB


def _decode_chunked(model, z, m, chunk_rows):
    """model.decode(z, m) in slices of chunk_rows, yielding (first row, decoded slice)."""
    step = max(1, int(chunk_rows))
    for r0 in range(0, z.shape[0], step):
        yield r0, model.decode(z[r0:r0 + step], m[r0:r0 + step])


def _decode_all(model, z, m, chunk_rows):
    """model.decode(z, m) of all rows, decoded in slices into one output."""
    out = None
    for r0, part in _decode_chunked(model, z, m, chunk_rows):
        if out is None:
            out = torch.empty((z.shape[0],) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
        out[r0:r0 + part.shape[0]].copy_(part)
    return out


def _require_eval(models):
    for mdl in models:
        if mdl.training:
            raise RuntimeError("vessel.analysis: put the model in eval mode first (model.eval()), as the reference consumers do")


@torch.no_grad()
def feature_importance(model, z, m, delta=1.0, features=None, chunk_rows=DEFAULT_CHUNK_ROWS):
    """Replaces analyze_vessel.py:68-121 (analyze_feature_importance): for each feature f, the mean over the N samples of
    ||decode(z, m + delta e_f) - decode(z, m)||_2 (the whole image flattened, :115-116).  z [N, Z] and m [N, M] are the caller's draws (the
    reference draws both with randn, :84-87).  One base decode per sample, the N x F perturbed rows decoded in chunks of chunk_rows, each chunk's
    norms taken against its base rows by cvae_row_diff_norms (ref = the sample index) — no perturbed image outlives its chunk.
    Returns [F] fp32 in the order of `features` (default: all M)."""
    _require_eval([model])
    N, M = m.shape
    features = list(range(M)) if features is None else [int(f) for f in features]
    base = _decode_all(model, z, m, chunk_rows)
    F = len(features)
    z_p = z.repeat(F, 1)                                           # rows ordered (feature, sample)
    m_p = m.repeat(F, 1)
    for i, f in enumerate(features):
        m_p[i * N:(i + 1) * N, f] += delta
    ref = torch.arange(N, device=z.device, dtype=torch.int64).repeat(F)
    l2 = torch.empty(F * N, dtype=torch.float32, device=z.device)
    for r0, part in _decode_chunked(model, z_p, m_p, chunk_rows):
        l2[r0:r0 + part.shape[0]] = ops.row_diff_norms(part, base, ref[r0:r0 + part.shape[0]])[0]
    return l2.view(F, N).mean(dim=1)


@torch.no_grad()
def ensemble_reconstruction(models, x, m, t, eps=None):
    """Replaces ensemble_reconstruction.py:57-89: the eval-mode reconstruction of every fold model on one batch, then the element-wise mean and
    unbiased std over the models (torch.stack(...).mean(0) / .std(0), :86-89) by cvae_stack_mean_std.  Each reconstruction is
    decode(reparameterize(encode(x, m, t)), m), forward's own composition (models.py:142-166); eps [B, Z] shared by all models, or None: each
    model draws its own, as each reference forward does.  Up to 16 models; one model gives a NaN std, as torch does."""
    _require_eval(models)
    recons = []
    for mdl in models:
        mu, logvar = mdl.encode(x, m, t)
        recons.append(mdl.decode(mdl.reparameterize(mu, logvar, eps), m))
    return ops.stack_mean_std(recons)


@torch.no_grad()
def z_permutation_grid(models, x, m, t, scale=1.0, chunk_rows=DEFAULT_CHUNK_ROWS):
    """Replaces check_mechanism_z_perm.py:100-130: grid[i, j] = mean over the models of decode(z = scale * mu_j, m_i) — M from sample i (row), Z from
    sample j (column), mu_j the encoder mean of sample j (:115-119).  The reference makes n^2 batch-1 forward + decode pairs per model; here each
    model makes one encode of the n samples and one n^2-row decode (in chunks), and the models' grids are averaged by cvae_stack_mean_std.
    Returns [n, n, 1, 768, 1280]."""
    _require_eval(models)
    n = x.shape[0]
    ii = torch.arange(n, device=x.device).repeat_interleave(n)      # row i * n + j: m from i, z from j
    jj = torch.arange(n, device=x.device).repeat(n)
    grids = []
    for mdl in models:
        mu, _logvar = mdl.encode(x, m, t)
        z_rows, m_rows = (mu * scale)[jj].contiguous(), m[ii].contiguous()
        grids.append(_decode_all(mdl, z_rows, m_rows, chunk_rows))
    mean, _std = ops.stack_mean_std(grids)
    return mean.view(n, n, *mean.shape[1:])
