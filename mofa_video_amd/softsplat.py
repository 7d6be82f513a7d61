"""Drop-in for the reference warp op ``softsplat(tenIn, tenFlow, tenMetric, strMode)``
(MOFA-Video-Traj/models/softsplat.py:232-274; kernel :284-345) on MI355X, differentiable as the reference's.

The inference path uses ``'avg'`` with ``tenMetric=None`` only (every call site: svdxt_..._norefine.py:231,
Hybrid/models/ldmk_ctrlnet.py:300, Hybrid/models/traj_ctrlnet.py:240): it runs the deterministic gather kernel on fp16
features (the adapter's features are fp16 and the reference rounds the result back to fp16, so the rounding points
coincide).  ``'sum'`` runs the literal fp32 atomicAdd scatter; the metric-weighted modes ``'linear'`` / ``'soft'`` and the
``-addeps`` / ``-zeroeps`` / ``-clipeps`` suffixes (softsplat.py:243-270) are that scatter between a weighting and a
normalising kernel, all in fp32 as the reference's ``custom_fwd(cast_inputs=torch.float32)``.  Same assertions as the
reference; no CPU path (the reference asserts on non-CUDA tensors too, softsplat.py:347-348).

Training (the reference's Training/ tree binds the same op): when grad mode is on and an input requires grad, the call records
an autograd node whose backward runs the HIP backward kernels (include/mofa_hip.h, mofa_softsplat_grad_f32) -- the raw sum
through ``softsplat_func`` (softsplat_func.backward, softsplat.py:349-524), the normalised modes through the mode prep and the
normalisation as well.  Gradients are fp32 (cast back to an input's dtype by autograd) and reproducible bit for bit; the
forward values are the same with and without grad tracking ('avg' stays the fp16 gather; its backward treats that rounding as
identity).  Double backward is not supported.

``GATHER_F32`` (initial value: ``MOFA_SOFTSPLAT_GATHER_F32=1`` in the environment; read at every call; off by default) runs every
mode as one call of the deterministic fp32 gather (include/mofa_hip.h, mofa_softsplat_gather_f32) instead: fp32 end to end as the
reference computes it, the same bits in every run and with or without grad tracking, and the normaliser it returns saves the
'avg' backward its second CSR build.  With the switch off, ``torch.use_deterministic_algorithms(True)`` moves the modes that would
use the atomicAdd scatter onto that path; 'avg' keeps its fp16 gather, which is deterministic already.
"""
import os

import torch
from torch.autograd.function import once_differentiable

from . import ops

GATHER_F32 = os.environ.get("MOFA_SOFTSPLAT_GATHER_F32") == "1"


def _use_gather_f32(strMode, gather_f32, deterministic):
    """whether a mode's forward is the fp32 gather: always with the switch; under torch's deterministic flag, every mode but 'avg'"""
    return bool(gather_f32) or (bool(deterministic) and strMode != 'avg')


def _prep(strMode):
    """the mode prep of mofa_softsplat_grad_f32: 'avg' [I | 1], 'linear*' [I * m | m], 'soft*' [I e^m | e^m]; 'avg-<suffix>' I"""
    return 1 if strMode == 'avg' else {'linear': 2, 'soft': 3}.get(strMode.split('-')[0], 0)


def _eps_mode(strMode):
    parts = strMode.split('-')
    return 0 if len(parts) == 1 or parts[1] == 'addeps' else {'zeroeps': 1, 'clipeps': 2}.get(parts[1], 3)


def _splat(tenIn, tenFlow, tenMetric, strMode, want_norm=False):
    """the forward of every mode -> (output, the splatted normaliser channel [N,1,H,W] or None: 'sum*', and 'avg' on the fp16 path);
    want_norm: the fp32 gather returns the normaliser as well (its output does not depend on that)"""
    N, C, H, W = tenIn.shape
    if _use_gather_f32(strMode, GATHER_F32, torch.are_deterministic_algorithms_enabled()):
        prep, normalize = _prep(strMode), strMode.split('-')[0] != 'sum'
        return ops.softsplat_gather_f32(tenIn.float().contiguous(), tenFlow.float().contiguous(),
                                        tenMetric.float().contiguous() if prep >= 2 else None, prep, normalize,
                                        _eps_mode(strMode) if normalize else 0, want_norm=want_norm and normalize)
    if strMode.split('-')[0] == 'sum':       # 'sum' and 'sum-<suffix>': the raw splat, nothing is normalised (softsplat.py:252)
        return ops.softsplat_scatter_f32(tenIn.float().contiguous(), tenFlow.float().contiguous()), None
    if strMode == 'avg':
        Cp = (C + 7) // 8 * 8
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=tenIn.device)
        for n in range(N):
            tok = ops.nchw_to_tokens(tenIn[n:n + 1].float().contiguous(), ld=Cp)
            w = ops.softsplat_avg_tokens(tok, tenFlow[n:n + 1].float().contiguous(), H, W)
            out[n:n + 1] = ops.tokens_to_nchw(w, 1, C, H, W)
        return out, None
    # 'linear' / 'soft' (and 'avg-<suffix>', for which the reference concatenates nothing: softsplat.py:243 tests strMode == 'avg')
    parts = strMode.split('-')
    t = tenIn.float().contiguous()
    if parts[0] == 'linear':
        t = ops.softsplat_weight_f32(t, tenMetric.float().contiguous(), 1)
    elif parts[0] == 'soft':
        t = ops.softsplat_weight_f32(t, tenMetric.float().contiguous(), 2)
    summed = ops.softsplat_scatter_f32(t, tenFlow.float().contiguous())
    return ops.softsplat_normalize_f32(summed, _eps_mode(strMode)), summed[:, -1:]


class softsplat_func(torch.autograd.Function):
    """the reference's raw sum splat (softsplat.py:277-527): ``apply(tenIn, tenFlow)``, fp32 under autocast, differentiable in
    both inputs"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, tenIn, tenFlow):
        assert tenIn.is_cuda and tenFlow.is_cuda, "softsplat: CUDA/HIP tensors required (as in the reference)"
        tenIn, tenFlow = tenIn.float().contiguous(), tenFlow.float().contiguous()
        assert tenFlow.shape == (tenIn.shape[0], 2, tenIn.shape[2], tenIn.shape[3])
        out = _splat(tenIn, tenFlow, None, 'sum')[0]
        ctx.save_for_backward(tenIn if ctx.needs_input_grad[1] else None, tenFlow)
        return out

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, tenOutgrad):
        tenIn, tenFlow = ctx.saved_tensors
        dI, dF, _ = ops.softsplat_grad_f32(tenOutgrad.float(), tenFlow, tenOutgrad.shape[1], 0, tenIn=tenIn,
                                           want_in=ctx.needs_input_grad[0], want_flow=ctx.needs_input_grad[1])
        return dI, dF


class _softsplat_normalized(torch.autograd.Function):
    """'avg', 'avg-<suffix>', 'linear*', 'soft*': the forward of ``softsplat`` unchanged; the backward is the prologue
    (1 / normaliser and the normaliser channel's gradient) and one gather over the source pixels"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, tenIn, tenFlow, tenMetric, strMode):
        out, norm = _splat(tenIn, tenFlow, tenMetric, strMode, want_norm=True)
        need_in = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ctx.strMode, ctx.C = strMode, tenIn.shape[1]
        ctx.save_for_backward(tenIn.float().contiguous() if need_in else None, tenFlow.float().contiguous(),
                              tenMetric.float().contiguous() if tenMetric is not None else None, out,
                              norm.contiguous() if norm is not None else None)
        return out

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, tenOutgrad):
        tenIn, tenFlow, tenMetric, out, norm = ctx.saved_tensors
        g = tenOutgrad.float().contiguous()
        if norm is None:                      # 'avg' on the fp16 path (the fp32 gather returned its normaliser with the output)
            norm = ops.softsplat_norm_f32(tenFlow)
        inv, glast = ops.softsplat_grad_prologue_f32(g, out, norm, _eps_mode(ctx.strMode))
        dI, dF, dm = ops.softsplat_grad_f32(g, tenFlow, ctx.C, _prep(ctx.strMode), tenIn=tenIn, metric=tenMetric, inv=inv, glast=glast,
                                            want_in=ctx.needs_input_grad[0], want_flow=ctx.needs_input_grad[1],
                                            want_metric=ctx.needs_input_grad[2])
        return dI, dF, dm, None


def softsplat(tenIn: torch.Tensor, tenFlow: torch.Tensor, tenMetric: torch.Tensor, strMode: str):
    assert strMode.split('-')[0] in ['sum', 'avg', 'linear', 'soft']
    if strMode == 'sum':
        assert tenMetric is None
    if strMode == 'avg':
        assert tenMetric is None
    if strMode.split('-')[0] == 'linear':
        assert tenMetric is not None
    if strMode.split('-')[0] == 'soft':
        assert tenMetric is not None
    assert tenIn.is_cuda and tenFlow.is_cuda, "softsplat: CUDA/HIP tensors required (as in the reference)"
    N, C, H, W = tenIn.shape
    assert tenFlow.shape == (N, 2, H, W)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (tenIn, tenFlow, tenMetric)):
        if strMode.split('-')[0] == 'sum':
            return softsplat_func.apply(tenIn, tenFlow)
        return _softsplat_normalized.apply(tenIn, tenFlow, tenMetric, strMode)
    return _splat(tenIn, tenFlow, tenMetric, strMode)[0]
