"""More than 32 frames per forward pass, end to end: the pipelines built with ``max_temporal_frames=...`` against the fp32 CPU
oracle on tiny models (the configurations of tests/test_pipeline_api_gpu.py, at 128 x 128 and 2 steps so that the oracle stays
quick at 40 ... 65 frames).  Latents after the loop and decoded frames: tensor-wide rel-L2 and the worst single frame's rel-L2
both under the project's stated 2e-2 (tests/test_model_gpu.py)."""
import pytest
import torch

from helpers import (LDMK_CN, LDMK_UNET, TINY, TINY_CN, TINY_VAE, frame_errors, oracle_models, synthetic_inputs,
                     synthetic_landmarks)

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 128, 128
STEPS, CHUNK = 2, 8
BAR = 2e-2


@pytest.fixture(scope="module")
def tiny():
    from mofa_video_amd.adapter import FlowControlNet
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    from mofa_video_amd.vae import AutoencoderKLTemporalDecoder
    ou, oc, ov, sdu, sdc, sdv = oracle_models(TINY, seed=0, vae_cfg=TINY_VAE, cn_cfg=TINY_CN)
    mods = dict(vae=AutoencoderKLTemporalDecoder(sdv, TINY_VAE, DEV), unet=UNetSpatioTemporalConditionControlNetModel(sdu, TINY, DEV),
                controlnet=FlowControlNet(sdc, TINY_CN, DEV), scheduler=EulerDiscreteScheduler())
    return mods, (ou, oc, ov)


@pytest.fixture(scope="module")
def ldmk():
    from mofa_video_amd import schema
    from mofa_video_amd.adapter import LandmarkFlowControlNet
    from mofa_video_amd.unet import UNetSpatioTemporalConditionControlNetModel
    from mofa_video_amd.vae import AutoencoderKLTemporalDecoder
    from oracle.ldmk import LandmarkFlowControlNet as OLdmk
    from oracle.unet import UNetSpatioTemporalConditionControlNetModel as OUnet
    from oracle.vae import AutoencoderKLTemporalDecoder as OVae
    sdl = schema.synthetic_state_dict(schema.ldmk_controlnet_schema(LDMK_CN), seed=11)
    sdu = schema.synthetic_state_dict(schema.unet_schema(LDMK_UNET), seed=10)
    sdv = schema.synthetic_state_dict(schema.vae_decoder_schema(**TINY_VAE), seed=13)
    of, ou, ov = OLdmk(**LDMK_CN), OUnet(**LDMK_UNET), OVae(**TINY_VAE)
    of.load_state_dict({k: t.float() for k, t in sdl.items()})
    ou.load_state_dict({k: t.float() for k, t in sdu.items()})
    ov.load_state_dict({k: t.float() for k, t in sdv.items()})
    return (of.eval(), ou.eval(), ov.eval(), LandmarkFlowControlNet(sdl, LDMK_CN, DEV),
            UNetSpatioTemporalConditionControlNetModel(sdu, LDMK_UNET, DEV), AutoencoderKLTemporalDecoder(sdv, TINY_VAE, DEV))


def _compare(what, lat, ref_lat, frames, ref_frames):
    el, ef = frame_errors(lat, ref_lat, dim=1), frame_errors(frames, ref_frames, dim=2)
    print(f"LONG-CLIP {what}: latents rel-L2 {el.tensor:.3e}, worst frame {max(el.rel):.3e} (frame {el.worst_rel}); "
          f"decoded frames rel-L2 {ef.tensor:.3e}, worst frame {max(ef.rel):.3e} (frame {ef.worst_rel})")
    assert tuple(lat.shape) == tuple(ref_lat.shape) and tuple(frames.shape) == tuple(ref_frames.shape)
    assert el.tensor < BAR and max(el.rel) < BAR, (what, el.summary())
    assert ef.tensor < BAR and max(ef.rel) < BAR, (what, ef.summary())


@pytest.mark.parametrize("T,limit", [(40, 64), (65, 128)])
def test_flow_pipeline_long_clip_vs_oracle(tiny, T, limit):
    from mofa_video_amd.pipeline import FlowControlNetPipeline
    from mofa_video_amd.vae import decode_latents
    from oracle.pipeline import denoise
    from oracle.scheduler import EulerDiscreteScheduler as OSch
    from oracle.vae import decode_latents as odecode
    mods, (ou, oc, ov) = tiny
    inp = synthetic_inputs(T, H, W, cross_dim=TINY["cross_attention_dim"], seed=52)
    with torch.no_grad():
        ref_lat = denoise(ou, oc, OSch(), inp["latents"], inp["image_latents"], inp["image_embeddings"], inp["cond"], inp["flow"],
                          num_inference_steps=STEPS)
        ref_frames = odecode(ov, ref_lat, T, decode_chunk_size=CHUNK)
    kw = dict(controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], height=H, width=W, num_frames=T,
              num_inference_steps=STEPS, decode_chunk_size=CHUNK, latents=inp["latents"], output_type="latent",
              image_embeddings=inp["image_embeddings"], image_latents=inp["image_latents"])
    with pytest.raises(ValueError, match="temporal attention"):          # the default limit is unchanged
        FlowControlNetPipeline(**mods)(None, **kw)
    pipe = FlowControlNetPipeline(**mods, max_temporal_frames=limit)
    lat = pipe(None, **kw).frames
    frames = decode_latents(mods["vae"], lat, T, CHUNK)
    _compare(f"flow pipeline T={T}", lat, ref_lat, frames, ref_frames)


def test_keypoint_loop_long_windows_vs_oracle(ldmk):
    from mofa_video_amd.pipeline import KeypointFlowControlNetPipeline
    from mofa_video_amd.scheduler import EulerDiscreteScheduler
    from mofa_video_amd.vae import decode_latents
    from oracle.pipeline import denoise_keypoint_loop
    from oracle.scheduler import EulerDiscreteScheduler as OSch
    from oracle.vae import decode_latents as odecode
    of, ou, ov, hf, hu, hv = ldmk
    N, win, stride = 61, 40, 21
    inp = synthetic_inputs(N, H, W, cross_dim=LDMK_CN["cross_attention_dim"], seed=56)
    lm = synthetic_landmarks(N, H, W, seed=57)
    with torch.no_grad():
        ref_lat = denoise_keypoint_loop(ou, of, OSch(), inp["latents"], inp["image_latents"], inp["image_embeddings"], inp["cond"],
                                        inp["flow"], lm, window_size=win, stride=stride, num_inference_steps=STEPS,
                                        reuse_identical_views=True)
        ref_frames = odecode(ov, ref_lat, N, decode_chunk_size=CHUNK)
    pipe = KeypointFlowControlNetPipeline(unet=hu, controlnet=hf, scheduler=EulerDiscreteScheduler(), max_temporal_frames=64)
    lat = pipe(None, controlnet_condition=inp["cond"], controlnet_flow=inp["flow"], landmarks=lm.to(DEV), window_size=win,
               stride=stride, height=H, width=W, num_frames=N, num_inference_steps=STEPS, latents=inp["latents"],
               output_type="latent", image_embeddings=inp["image_embeddings"], image_latents=inp["image_latents"]).frames
    frames = decode_latents(hv, lat, N, CHUNK)
    _compare(f"keypoint loop N={N} window={win} stride={stride}", lat, ref_lat, frames, ref_frames)
