"""The ViT recipes' training step as one HIP graph: causal_vit_train_step, the vessel recipe's single step on CausalViTVAE.forward_train
(its ViTVAE counterpart, vit_vae_train_step, lives next to train_vit_vae in models.py), and GraphedViTTrainStep, which captures either step once and
replays it.  What makes the capture possible is that nothing in a step reaches the host: Adam's step count (FusedAdam(device_step=True)), the heads'
BatchNorm1d counters and, with dropout, the Philox key counter (ops.DeviceDropoutKeys) all live on the device and advance inside the graph."""
import torch

from .. import ops
from .._lib import CvaeError, require_gpu
from ..graph import _capture
from .causal import CausalViTVAE
from .models import ViTVAE, _check_graph_optimizer, vit_vae_train_step


def causal_vit_train_step(model, optimizer, x, m, t, eps=None, beta=0.5, lambda_morph=1.0, max_norm=5.0):
    """vessel.train.train_step's recipe on CausalViTVAE.forward_train (model(x, m, t) is the no_grad eval forward, so that function does not fit):
    zero_grad -> forward_train -> vessel loss -> backward -> clip_grad_norm_(max_norm) -> step.  Needs model.train_adapters(...) first, as forward_train
    does.  With a FusedAdam the norm and the clip coefficient stay on the device and the Adam launch applies the coefficient; any other optimizer gets
    torch's in-place clip.  Returns (loss, recon, kld, morph) as 0-dim device tensors; no host sync."""
    from ..optim import FusedAdam, clip_grad_norm_
    from ..vessel.train import loss_function, total_loss
    optimizer.zero_grad(set_to_none=True)
    out = model.forward_train(x, m, t, eps=eps)
    with ops.zero_pool(8, x):                                # the loss terms' zeroed scalar outputs: one fill launch instead of one each
        recon, kld, morph, sparsity = loss_function(out[0], x, out[1], m, out[2], out[3], out[4], out[5])
        loss = total_loss(recon, kld, morph, sparsity, beta=beta, lambda_morph=lambda_morph)
    ops.backward_from(loss)
    params = [p for p in model.parameters() if p.grad is not None]
    if isinstance(optimizer, FusedAdam):
        _sq, coef = clip_grad_norm_(params, max_norm, scale_grads=False)
        optimizer.step(grad_scale=coef)
    else:
        torch.nn.utils.clip_grad_norm_(params, max_norm=max_norm)
        optimizer.step()
    return loss.detach(), recon.detach(), kld.detach(), morph.detach()


class GraphedViTTrainStep:
    """One training step of a ViTVAE (batch = (x,): vit_vae_train_step) or a CausalViTVAE (batch = (x, m, t): causal_vit_train_step) captured as one HIP
    graph; `recipe` holds that function's keywords (beta, ...).  The batch tensors are cloned into static buffers (self.batch).
    eps=None: every replay draws its noise with torch's generator into the static buffer self.eps, inside the graph; an eps tensor makes that buffer
    an input that __call__(..., eps=...) refills.  The optimizer must be FusedAdam(device_step=True); with the model's dropout on, the keys move to
    the device (use_device_dropout_keys()).
    Constructing it does not train: parameters, buffers (the heads' BatchNorm1d statistics and counters), Adam's moments and step count and the dropout
    step are copied before the `warmup` eager steps (allocator, lazy kernel attributes, Adam state; on a side stream) and, after the capture, written
    back in place — the graph replays against those very tensors — so the first replay is step 0 of the run.
    __call__(*batch, eps=None) -> the step function's result (static 0-dim tensors, rewritten by the next replay)."""

    def __init__(self, model, optimizer, batch, *, eps=None, warmup=3, **recipe):
        _check_graph_optimizer("GraphedViTTrainStep", optimizer)
        causal = isinstance(model, CausalViTVAE)
        if not causal and not isinstance(model, ViTVAE):
            raise CvaeError(f"GraphedViTTrainStep: a ViTVAE or a CausalViTVAE expected, got {type(model).__name__}")
        batch = tuple(batch)
        if len(batch) != (3 if causal else 1):
            raise CvaeError(f"GraphedViTTrainStep: batch must be {'(x, m, t)' if causal else '(x,)'} for a {type(model).__name__}, got {len(batch)} tensors")
        if int(warmup) < 1:
            raise CvaeError("GraphedViTTrainStep: warmup >= 1 expected (Adam's moments must exist before the capture, or every replay would zero them)")
        require_gpu(*batch, eps, *model.parameters())
        self.model, self.opt, self.recipe = model, optimizer, dict(recipe)
        self._fn = causal_vit_train_step if causal else vit_vae_train_step
        encoder = model.backbone if causal else model
        if encoder._dropout:
            encoder.use_device_dropout_keys()
        self.batch = tuple(b.clone() for b in batch)
        B, Z = batch[0].shape[0], (model.my_z_dim if causal else model.latent_dim)
        if eps is not None and (tuple(eps.shape) != (B, Z) or eps.dtype != torch.float32):
            raise CvaeError(f"GraphedViTTrainStep: eps must be a float32 [{B}, {Z}] matrix, got {tuple(eps.shape)} {eps.dtype}")
        self._draw = eps is None
        self.eps = torch.zeros(B, Z, dtype=torch.float32, device=batch[0].device) if eps is None else eps.clone()

        keep = self._snapshot(encoder)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(int(warmup)):
                self._step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with _capture(self.graph):
            self.out = self._step()
        self._restore(encoder, keep)

    def _step(self):
        if self._draw:
            self.eps.normal_()
        return self._fn(self.model, self.opt, *self.batch, eps=self.eps, **self.recipe)

    # ---- the state a step changes, copied before the warm-up and written back in place after the capture --------------------------------
    def _snapshot(self, encoder):
        opt, keys = self.opt, encoder.dropout_keys
        params = [p for g in opt.param_groups for p in g["params"]]
        return {
            "tensors": [(t, t.detach().clone()) for t in list(self.model.parameters()) + list(self.model.buffers())],
            "adam": {p: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state[p].items()} for p in params if opt.state.get(p)},
            "adam_step": None if opt._step_dev is None else opt._step_dev.clone(),
            "drop": keys.counter.clone() if isinstance(keys, ops.DeviceDropoutKeys) else keys.step,
        }

    @torch.no_grad()
    def _restore(self, encoder, keep):
        opt, keys = self.opt, encoder.dropout_keys
        for t, was in keep["tensors"]:
            t.copy_(was)
        for p, st in opt.state.items():                      # moments born in the warm-up start from zero, as Adam's do; older ones from their copy
            was = keep["adam"].get(p)
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    st[k].zero_() if was is None else st[k].copy_(was[k])
            if "step" in st:
                st["step"] = 0 if was is None else was["step"]
        if opt._step_dev is not None:
            opt._step_dev.zero_() if keep["adam_step"] is None else opt._step_dev.copy_(keep["adam_step"])
        if isinstance(keys, ops.DeviceDropoutKeys):
            keys.counter.copy_(keep["drop"])
        else:
            keys.step = keep["drop"]
        torch.cuda.synchronize()

    def __call__(self, *batch, eps=None):
        """Replay one step; new inputs (same shapes) are copied into the static buffers first.  Returns the static result tensors."""
        if len(batch) not in (0, len(self.batch)):
            raise CvaeError(f"GraphedViTTrainStep: {len(self.batch)} batch tensors expected (or none: replay on the buffers as they are), got {len(batch)}")
        for dst, src in zip(self.batch, batch):
            dst.copy_(src, non_blocking=True)
        if eps is not None:
            if self._draw:
                raise CvaeError("GraphedViTTrainStep: this step draws its own noise (built with eps=None); build it with an eps tensor to pass one")
            self.eps.copy_(eps, non_blocking=True)
        self.graph.replay()
        return self.out
