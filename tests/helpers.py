"""Shared test fixtures: seeded synthetic weights (same fp16-rounded values on both sides) and synthetic
inputs of SURVEY.md 8(d) at reduced sizes the CPU oracle finishes in seconds."""
import math

import torch

from mofa_video_amd import schema

TINY = dict(block_out_channels=(64, 128, 256, 256), num_attention_heads=(1, 2, 4, 4), cross_attention_dim=128)
# the reference ControlNet trunk uses heads (5,10,10,20) -> head dim 128 at level 2; mirrored here (256 / 2)
TINY_CN = dict(TINY, num_attention_heads=(1, 2, 2, 4))
TINY_VAE = dict(block_out_channels=(64, 64, 128, 128))


# reduced configs for the landmark adapter / Hybrid / Keypoint cases: level 0 keeps 320 channels because the reference
# forward tests ``sample.shape[1] == 320`` literally (ldmk_ctrlnet.py:501); heads mirror (5,10,10,20) / (5,10,20,20)
LDMK_CN = dict(block_out_channels=(320, 128, 256, 256), num_attention_heads=(5, 2, 2, 4), cross_attention_dim=128)
LDMK_UNET = dict(block_out_channels=(320, 128, 256, 256), num_attention_heads=(5, 2, 4, 4), cross_attention_dim=128)


def synthetic_landmarks(T, H, W, seed=44):
    """pose images: sparse binary polylines-like pixels in [0,1], [1,T,3,H,W]"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(1, T, 3, H, W, generator=g) < 0.02).float()


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


class FrameErrors:
    """per-frame figures of a product tensor against its reference (``frame_errors``): ``rel[i]`` = rel-L2 of frame i,
    ``maxabs[i]`` = max|out - ref| / max|ref| over frame i, ``worst_rel`` / ``worst_abs`` = the frame numbers (``f0 + i``) where
    they peak, ``worst_elem`` = index of the largest |out - ref| of the whole tensor, ``tensor`` = the tensor-wide rel-L2"""

    def __init__(self, rel, maxabs, f0, worst_elem, tensor):
        self.rel, self.maxabs, self.f0, self.worst_elem, self.tensor = rel, maxabs, f0, worst_elem, tensor
        self.worst_rel = f0 + max(range(len(rel)), key=lambda i: rel[i])
        self.worst_abs = f0 + max(range(len(maxabs)), key=lambda i: maxabs[i])

    def frame(self, f):
        """(rel-L2, max-abs ratio) of frame ``f`` (a frame number, f0 counted)"""
        return self.rel[f - self.f0], self.maxabs[f - self.f0]

    def summary(self):
        return (f"tensor rel-L2 {self.tensor:.3e}; per frame rel-L2 max {max(self.rel):.3e} (frame {self.worst_rel}), "
                f"max-abs / max|ref| max {max(self.maxabs):.3e} (frame {self.worst_abs}); worst element {self.worst_elem}")


def frame_errors(out, ref, dim=1, f0=0):
    """per-frame rel-L2 and max|delta| / max|ref| of ``out`` against ``ref`` along the frame axis ``dim`` (fp64, on the tensors'
    device); frame numbers start at ``f0`` (the first frame of a shard).  Non-finite values give non-finite figures."""
    assert tuple(out.shape) == tuple(ref.shape), (tuple(out.shape), tuple(ref.shape))
    o = out.detach().to(ref.device, torch.float64).movedim(dim, 0)
    r = ref.detach().to(torch.float64).movedim(dim, 0)
    n = o.shape[0]
    d = (o - r).reshape(n, -1)
    r = r.reshape(n, -1)
    rel = (d.norm(dim=1) / (r.norm(dim=1) + 1e-30)).tolist()
    dabs = d.abs()
    dabs = torch.where(torch.isnan(dabs), torch.full_like(dabs, math.inf), dabs)    # (a NaN is the worst element there is)
    maxabs = (dabs.amax(dim=1) / (r.abs().amax(dim=1) + 1e-30)).tolist()
    k = int(dabs.reshape(-1).argmax())
    i, j = divmod(k, d.shape[1])                                                     # (frame, flat index inside the frame)
    rest = list(out.shape)
    del rest[dim]
    idx = list(_unravel(j, rest))
    idx.insert(dim, f0 + i)
    tensor = float(d.norm() / (r.norm() + 1e-30))
    return FrameErrors(rel, maxabs, f0, tuple(idx), tensor)


def _unravel(j, shape):
    idx = []
    for s in reversed(shape):
        j, m = divmod(j, s)
        idx.append(m)
    return reversed(idx)


def check_frames(out, ref, rel_tol, abs_tol, dim=1, f0=0, what="", named=()):
    """asserts rel-L2 < rel_tol and max|delta| / max|ref| < abs_tol for EVERY frame of ``out`` against ``ref`` (frame axis
    ``dim``, frame numbers from ``f0``); prints the worst figures and those of the frames in ``named``; returns the FrameErrors.
    The failure message names every frame out of bounds and the worst element."""
    e = frame_errors(out, ref, dim, f0)
    print(f"{what}: {e.summary()}")
    for f in named:
        r, a = e.frame(f)
        print(f"{what}: frame {f}: rel-L2 {r:.3e}, max-abs / max|ref| {a:.3e}")
    bad = [(f0 + i, r, a) for i, (r, a) in enumerate(zip(e.rel, e.maxabs)) if not (r < rel_tol and a < abs_tol)]
    assert not bad, (f"{what}: " + "; ".join(f"frame {f} rel-L2 {r:.3e}, max-abs / max|ref| {a:.3e}" for f, r, a in bad) +
                     f" (bars {rel_tol:g} / {abs_tol:g}); worst element {e.worst_elem}")
    return e


def oracle_models(cfg=None, seed=0, vae_cfg=None, cn_cfg=None):
    """returns (oracle_unet, oracle_controlnet, oracle_vae, sd_unet, sd_ctrl, sd_vae) with fp16-valued weights"""
    from oracle.controlnet import FlowControlNet
    from oracle.unet import UNetSpatioTemporalConditionControlNetModel
    from oracle.vae import AutoencoderKLTemporalDecoder
    kw = cfg or {}
    ckw = cn_cfg if cn_cfg is not None else kw
    sdu = schema.synthetic_state_dict(schema.unet_schema(cfg), seed=seed)
    sdc = schema.synthetic_state_dict(schema.controlnet_schema(cn_cfg if cn_cfg is not None else cfg), seed=seed + 1)
    vkw = vae_cfg or {}
    sdv = schema.synthetic_state_dict(schema.vae_decoder_schema(**vkw), seed=seed + 2)
    u = UNetSpatioTemporalConditionControlNetModel(**kw)
    c = FlowControlNet(**ckw)
    v = AutoencoderKLTemporalDecoder(**vkw)
    u.load_state_dict({k: t.float() for k, t in sdu.items()})
    c.load_state_dict({k: t.float() for k, t in sdc.items()})
    v.load_state_dict({k: t.float() for k, t in sdv.items()})
    return u.eval(), c.eval(), v.eval(), sdu, sdc, sdv


def synthetic_inputs(T, H, W, cross_dim=1024, seed=42):
    """SURVEY 8(d) config-2 style inputs: one Gaussian-bump trajectory flow growing linearly over frames."""
    g = torch.Generator().manual_seed(seed)
    h, w = H // 8, W // 8
    latents = torch.randn(1, T, 4, h, w, generator=g)
    image_latents = torch.randn(1, 4, h, w, generator=g) / 0.18215
    image_embeddings = torch.randn(1, 1, cross_dim, generator=g)
    cond = torch.rand(1, 3, H, W, generator=g) * 2 - 1
    ys = torch.arange(H, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, W)
    sig = 0.15 * min(H, W)
    bump = torch.exp(-((xs - W / 2) ** 2 + (ys - H / 2) ** 2) / (2 * sig * sig))
    peak = torch.tensor([64.0 * W / 1024, 32.0 * H / 576])
    flow = torch.zeros(1, T - 1, 2, H, W)
    for i in range(T - 1):
        f = (i + 1) / (T - 1)
        flow[0, i, 0] = bump * peak[0] * f
        flow[0, i, 1] = bump * peak[1] * f
    il2 = torch.cat([torch.zeros_like(image_latents), image_latents])
    emb2 = torch.cat([torch.zeros_like(image_embeddings), image_embeddings])
    return dict(latents=latents, image_latents=il2, image_embeddings=emb2, cond=cond, flow=flow)
