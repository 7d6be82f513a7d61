"""One ``name sha256`` line per pipeline configuration, over the bytes of what the public ``__call__`` returns on the tiny seeded
models of tests/test_pipeline_api_gpu.py (256 x 256, h = w = 32).  Two revisions of the host code that print the same lines on
the same library computed the same bits: the proof a refactor of pipeline.py is checked by.  Virtual-rank cases (threads over
``ThreadWorld``) hash every rank's result; a sharded decode returns (first frame, frames) chunks, hashed in order.

    python tools/pipeline_fingerprint.py          (MOFA_HIP_LIB / PYTHONPATH select the library / the package under test)
"""
import hashlib
import os
import sys
import threading

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)                          # (appended: a package earlier on PYTHONPATH is the one under test)
sys.path.append(os.path.join(ROOT, "tests"))
from helpers import LDMK_CN, LDMK_UNET, TINY, TINY_CN, TINY_VAE, synthetic_inputs, synthetic_landmarks  # noqa: E402
from mofa_video_amd import parallel as P, pipeline as PL, schema  # noqa: E402
from mofa_video_amd.adapter import FlowControlNet, LandmarkFlowControlNet  # noqa: E402
from mofa_video_amd.scheduler import EulerDiscreteScheduler  # noqa: E402
from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel as UNet  # noqa: E402
from mofa_video_amd.vae import AutoencoderKLTemporalDecoder as VAE  # noqa: E402

DEV, T, H, W = "cuda", 3, 256, 256


def digest(x):
    h = hashlib.sha256()
    for part in (x if isinstance(x, list) else [(0, x)]):
        h.update(str(part[0]).encode())
        h.update(part[1].detach().float().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def ranks(world, fn):
    """fn(rank, ThreadWorld) on ``world`` virtual ranks -> their results"""
    tw, out, err = P.ThreadWorld(world), [None] * world, []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(r, tw)
        except Exception as e:  # noqa: BLE001
            err.append((r, repr(e)))
            for b in tw.barriers.values():
                b.abort()
    ths = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(600)
    if err:
        raise RuntimeError(err)
    return out


def main():
    sd = schema.synthetic_state_dict
    vae = VAE(sd(schema.vae_decoder_schema(**TINY_VAE), seed=2), TINY_VAE, DEV)
    flow_mods = dict(vae=vae, unet=UNet(sd(schema.unet_schema(TINY), seed=0), TINY, DEV),
                     controlnet=FlowControlNet(sd(schema.controlnet_schema(TINY_CN), seed=1), TINY_CN, DEV))
    face = LandmarkFlowControlNet(sd(schema.ldmk_controlnet_schema(LDMK_CN), seed=11), LDMK_CN, DEV)
    drag = FlowControlNet(sd(schema.controlnet_schema(LDMK_CN), seed=12), LDMK_CN, DEV)
    lunet = UNet(sd(schema.unet_schema(LDMK_UNET), seed=10), LDMK_UNET, DEV)
    inp = synthetic_inputs(T, H, W, cross_dim=TINY["cross_attention_dim"])
    mask = torch.zeros(1, 1, H, W)
    mask[:, :, H // 4:3 * H // 4, W // 4:3 * W // 4] = 1.0

    def common(i, n, steps, out):
        return dict(controlnet_condition=i["cond"], controlnet_flow=i["flow"], height=H, width=W, num_frames=n,
                    num_inference_steps=steps, decode_chunk_size=2, latents=i["latents"], output_type=out,
                    image_embeddings=i["image_embeddings"], image_latents=i["image_latents"])

    def flow(out, steps=2, par=None, attrs=(), ctor=(), **kw):
        pipe = PL.FlowControlNetPipeline(**flow_mods, scheduler=EulerDiscreteScheduler(), parallel=par, **dict(ctor))
        for k, v in attrs:
            setattr(pipe, k, v)
        return pipe(None, **common(inp, T, steps, out), **kw).frames

    def long_inputs(n):
        i = synthetic_inputs(n, H, W, cross_dim=LDMK_CN["cross_attention_dim"], seed=46)
        return i, synthetic_landmarks(n, H, W, seed=47).to(DEV), synthetic_inputs(n, H, W, cross_dim=128, seed=48)["flow"] * 0.5

    def hybrid(out="latent", par=None):
        i, lm, dflow = long_inputs(T)
        pipe = PL.HybridFlowControlNetPipeline(vae=vae, unet=lunet, face_controlnet=face, drag_controlnet=drag,
                                               scheduler=EulerDiscreteScheduler(), parallel=par)
        return pipe(None, **common(i, T, 2, out), landmarks=lm, drag_flow=dflow, mask=mask, ctrl_scale_traj=0.8,
                    ctrl_scale_ldmk=1.1).frames

    def keypoint(n, par=None, overlap=True, hyb=False, out="raw"):
        i, lm, dflow = long_inputs(n)
        pipe = PL.KeypointFlowControlNetPipeline(vae=vae, unet=lunet, controlnet=face, drag_controlnet=drag,
                                                 scheduler=EulerDiscreteScheduler(), parallel=par, overlap_decode=overlap)
        kw = dict(drag_flow=dflow, mask=mask, ctrl_scale_traj=0.8) if hyb else {}
        return pipe(None, **common(i, n, 2, out), landmarks=lm, window_size=4, stride=2, **kw).frames

    def halve(pipe, i, t, kw):
        return {"latents": kw["latents"] * 0.5} if i == 0 else {}
    cases = []
    for out in ("latent", "raw"):
        cases += [(f"flow/{out}", lambda out=out: flow(out)),
                  (f"flow/{out}/callback", lambda out=out: flow(out, callback_on_step_end=halve)),
                  (f"flow/{out}/round16", lambda out=out: flow(out, ctor=[("round_latents_to_fp16", True)])),
                  (f"flow/{out}/one-stream", lambda out=out: flow(out, attrs=[("overlap_adapter", False)])),
                  (f"flow/{out}/whole-decoder", lambda out=out: flow(out, attrs=[("split_decoder", False)])),
                  (f"flow/{out}/graph3", lambda out=out: flow(out, steps=3, attrs=[("graph_steps", True)])),
                  (f"hybrid/{out}", lambda out=out: hybrid(out))]
    for ov in (True, False):
        for hyb in (False, True):
            cases.append((f"keypoint/N8/overlap{int(ov)}/hybrid{int(hyb)}", lambda ov=ov, hyb=hyb: keypoint(8, None, ov, hyb)))
    cases.append(("keypoint/N4", lambda: keypoint(4)))
    fp = lambda w, n: (lambda r, tw: P.FrameParallel(P.Layout(w, r, n), P.ThreadComm(tw, r)))  # noqa: E731
    virt = []
    for w, out in ((2, "latent"), (2, "raw"), (4, "latent"), (4, "raw")):
        virt += [(f"flow/frame{w}/{out}", w, lambda r, tw, w=w, out=out: flow(out, par=fp(w, T)(r, tw))),
                 (f"hybrid/frame{w}/{out}", w, lambda r, tw, w=w, out=out: hybrid(out, par=fp(w, T)(r, tw)))]
    virt.append(("keypoint/N4/frame2", 2, lambda r, tw: keypoint(4, fp(2, 4)(r, tw), hyb=True)))
    for w in (2, 3):
        virt.append((f"keypoint/N10/window{w}", w, lambda r, tw, w=w: keypoint(10, P.WindowParallel(P.ThreadComm(tw, r), r, w))))
    virt.append(("keypoint/N8/frame2", 2, lambda r, tw: keypoint(8, fp(2, 4)(r, tw), hyb=True)))
    virt.append(("keypoint/N10/grouped4x2", 4,
                 lambda r, tw: keypoint(10, P.GroupedWindowParallel(P.ThreadComm(tw, r), r, 4, 2, 4), hyb=True)))
    for name, fn in cases:
        print(f"{name} {digest(fn())}", flush=True)
    for name, world, fn in virt:
        for r, res in enumerate(ranks(world, fn)):
            print(f"virtual:{name}/rank{r} {digest(res)}", flush=True)


if __name__ == "__main__":
    main()
