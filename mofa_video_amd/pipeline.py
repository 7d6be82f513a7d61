"""MI355X host mirrors of the reference pipelines: ``FlowControlNetPipeline`` (MOFA-Video-Traj/pipeline/pipeline.py:87-527),
``HybridFlowControlNetPipeline`` (MOFA-Video-Hybrid/pipeline/pipeline.py:293-507) and ``KeypointFlowControlNetPipeline``
(MOFA-Video-Keypoint/pipeline/svdxt_pipeline_ctrlnet_loop.py:289-511).

Same constructor modules, ``__call__`` signatures, defaults (``output_type="pil"``) and return types.  The denoise loops run
entirely in libmofa_hip.so on token-major fp16 activations:

    per call (``_prologue``): checks, image conditioning, schedule, initial latents, the adapter's condition image
    per clip (``_run_clip``; hoisted, timestep-invariant -- SURVEY F7/F11):
        adapter.prepare_condition  (cond CNN, first-frame pyramid, flow pyramids, 96 forward-splat warps)
        cross-attention row vectors and frame-position embeddings of every transformer layer (cached in the ``Ctx``s)
        scheduler.step_table       (sigma, sigma_next, timestep, 1 / sqrt(sigma^2 + 1) of every step: ONE upload, ``_clip_loop``)
    per step (``_Step``; with ``graph_steps`` the steps 1 .. n-1 are replays of ONE captured hipGraph, ``_clip_loop``):
        mofa_prepare_model_input_dev  (scale by 1/sqrt(sigma^2+1), concat image latents, both CFG halves; scalars: the table row)
        adapter trunk(s) -> 12 + 1 residuals (Hybrid: two adapters + mask blend) || UNet encoder; UNet decoder  (``_denoise_forward``)
        mofa_cfg_euler_step_dev       (CFG with per-frame guidance + v-prediction Euler step, fp32 latents, in place)
    decode (``_decode``): temporal VAE decoder, chunks of ``decode_chunk_size`` frames.
The Keypoint window loop (``_WindowLoop``) runs the same step body per window with the scheduler's numbers as host scalars
(mofa_prepare_model_input / mofa_cfg_euler_step) and averages the overlapping windows as ``WindowPlan`` says.

Within a step the adapter's ControlNet trunk(s) and the UNet's encoder half (conv_in, down blocks, mid block) do not depend
on each other (the residuals are added after the mid block): without frame sharding the trunks are enqueued on a second HIP
stream and the encoder on the caller's (``_denoise_forward``; ``overlap_adapter=False`` restores the single-stream order).  Every
launch is a grid of persistent one-per-CU workgroups, so the second stream's kernel takes exactly the CUs the first one's tail
round leaves idle, and one stream's launch gap is covered by the other's kernel: 3.0-4.4 % of a denoise step on one MI355X
(tools/two_stream_probe.py), bit-identical results (same kernels, same tiles, same order per stream).

Image conditioning (once per clip before the loop, pipeline.py:330-352) also runs on the library when the
pipeline holds an ``image_encoder`` (mofa_video_amd.clip) and a VAE with encoder weights: ``image`` is then the PIL image /
[1,3,H,W] tensor in [0, 1] of the reference call (mofa_video_amd/frontend.py).  Precomputed conditioning can be passed
instead through the keyword-only extensions ``image_embeddings`` ([1,1,1024] or [2,1,1024]) and ``image_latents``
([1,4,h,w] or [2,4,h,w]).

Reference quirks kept: ``added_time_ids`` is always [6, 128, 0.02] (pipeline.py:430-440); CFG is always on
(max_guidance_scale > 1).  Stated deviations: (1) the latents stay fp32 between steps unless the pipeline is built with
``round_latents_to_fp16=True`` (the reference's fp16 run rounds them every step, scheduling_..._karras_fix.py:520);
(2) random draws (initial latents, noise augmentation) come from ``torch.randn`` in fp32 on the generator's device, so a
seed does not reproduce the reference's fp16 CUDA draws -- pass ``latents=`` for reproducibility across implementations;
(3) the scheduler's unused per-step randn draw is not made (no effect on results).
"""
import collections
import contextlib
import functools
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Union

import numpy as np
import torch

from . import frontend, ops
from .blocks import Ctx, drive, run_lockstep
from .output import tensor2vid
from .vae import decode_latents


@dataclass
class FlowControlNetPipelineOutput:
    frames: Union[List, np.ndarray, torch.FloatTensor]
    controlnet_flow: Union[List, np.ndarray, torch.FloatTensor]


MAX_TEMPORAL_FRAMES = 32        # mofa_attn_temporal_f16 holds one clip's keys in one score tile: the default limit per forward pass
MAX_TEMPORAL_FRAMES_LONG = 128  # mofa_attn_temporal_long_f16 (four key tiles): what max_temporal_frames=... can raise it to
# ... and what it can be raised to under a temporal_window of radius <= STREAM_RADIUS and anchor <= STREAM_ANCHOR, which
# mofa_attn_temporal_stream_local_f16 runs with four key tiles in a ring.  That kernel takes 1024 frames; 256 is what the other
# launches of a denoise step were read for (the row and offset arithmetic at 2 x 256 x 9216 rows)
MAX_TEMPORAL_FRAMES_STREAM = 256
STREAM_RADIUS = STREAM_ANCHOR = 32
# temporal_stream=True lifts the window rule: above 128 frames a window beyond the ring's limits, and no window at all (dense, the
# reference's own arithmetic), run through mofa_attn_temporal_stream_f16 -- up to the same MAX_TEMPORAL_FRAMES_STREAM


def _temporal_window(value):
    """the ``temporal_window`` keyword -> None or (radius, anchor): an int is (radius, 1) -- frame 0, the conditioning frame,
    stays visible to every query.  anchor <= T is checked per call, where T is known"""
    def whole(x):
        return isinstance(x, int) and not isinstance(x, bool)
    if value is None:
        return None
    if whole(value) and 0 <= value:
        return (value, 1)
    if isinstance(value, (tuple, list)) and len(value) == 2 and all(whole(x) for x in value) and value[0] >= 0 \
            and 0 <= value[1] <= MAX_TEMPORAL_FRAMES_LONG:
        return (value[0], value[1])
    raise ValueError("temporal_window must be None, an integer radius >= 0 or (radius >= 0, anchor in 0 .. "
                     f"{MAX_TEMPORAL_FRAMES_LONG}), got {value!r}")


def _shards_frames(parallel):
    """does this ``parallel`` object shard the frames of a forward pass (FrameParallel, or the groups of a
    GroupedWindowParallel)?  A CFG split alone and WindowParallel do not"""
    lay = getattr(getattr(parallel, "frame", parallel), "lay", None)
    return lay is not None and bool(lay.sharded_frames)


GRAPH_STEPS_DEFAULT = os.environ.get("MOFA_GRAPH_STEPS", "0") == "1"


class _Shard:
    """what this rank computes of a T-frame clip (mofa_video_amd/parallel.py): frames [f0, f1), Bl CFG halves"""

    def __init__(self, par, T):
        self.par, self.T = par, T
        self.lay = par.lay if par is not None else None
        if self.lay is not None and self.lay.T != T:
            raise ValueError(f"the parallel Layout was built for {self.lay.T} frames, the clip has {T}")
        self.f0, self.f1 = (self.lay.f0, self.lay.f1) if self.lay is not None else (0, T)
        self.Tl = self.f1 - self.f0
        self.Bl = self.lay.B_loc if self.lay is not None else 2
        self.half = self.lay.half if self.lay is not None else None
        self.fpar = par if (self.lay is not None and self.lay.sharded_frames) else None
        self.world = self.lay.world if self.lay is not None else 1
        self.rank = self.lay.rank if self.lay is not None else 0

    def guidance(self, gmin, gmax):
        """the guidance scales of this shard's first and last frame: per-frame guidance is linear in the frame of the clip"""
        gspan = (gmax - gmin) / max(self.T - 1, 1)
        return gmin + gspan * self.f0, gmin + gspan * (self.f1 - 1)

    def gather(self, lat, h, w):
        """this shard's stepped latents [Tl,4,h,w] -> the clip's [T,4,h,w] on every rank"""
        if self.fpar is None:
            return lat
        return self.fpar.gather_frames(lat.reshape(self.Tl, 4 * h * w), 1).reshape(self.T, 4, h, w)


def _rows_of(tt, hf):                                                  # CFG half ``hf`` of a token tensor that holds both
    n = tt.shape[0] // 2
    return tt[hf * n:(hf + 1) * n]


class _Step:
    """THE denoise step of every loop: model input -> adapter trunk(s) + UNet -> CFG + Euler step, on this rank's CFG half /
    frames ``sh`` of a clip or window.  Holds the model-input buffer and what no step changes; ``adapters`` / ``c_un`` (the
    networks' per-clip caches) are arguments because the window loop keeps one set per window.  ``scal`` says where the
    scheduler's numbers come from: a row of the device step table (the ``_dev`` entry points read it on the device, which makes
    a step capturable) or the host scalars (timestep, sigma, sigma_next).  The two forms differ by up to 1 fp16 ulp in the
    model input (tests/test_kernels_gpu.py::test_device_scalar_scheduler_kernels), so a loop stays with the form it has."""

    def __init__(self, pipe, sh, il, emb, networks, masks, h, w, g0, g1, round16=False):
        self.pipe, self.sh, self.il, self.emb, self.masks, self.h, self.w, self.g0, self.g1 = pipe, sh, il, emb, masks, h, w, g0, g1
        self.round16 = round16
        self.added_time_ids = torch.tensor([[6.0, 128.0, 0.02]] * 2, dtype=torch.float32, device=pipe.device)   # :430-440
        rows = sh.Tl * h * w
        in_ld = max(net.in_ld for net in [pipe.unet] + list(networks))
        self.x_in = torch.zeros((2 * rows, in_ld), dtype=torch.float16, device=pipe.device)
        self.x_loc = self.x_in if sh.Bl == 2 else self.x_in[sh.half * rows:(sh.half + 1) * rows]

    def __call__(self, lat, scal, adapters, c_un):
        """steps ``lat`` fp32 [Tl,4,h,w] in place"""
        sh, table = self.sh, torch.is_tensor(scal)
        if table:
            ops.prepare_model_input_dev(lat, self.il, self.x_in, scal)
            t = scal[2:2 + sh.Bl]
        else:
            t, sigma, sigma_next = scal
            ops.prepare_model_input(lat, self.il, self.x_in, sigma)
        noise = self.pipe._denoise_forward(self.x_loc, t, self.emb, self.added_time_ids, sh.Bl, sh.Tl, sh.half, sh.fpar, self.h, self.w,
                                           adapters, c_un, self.masks)
        if sh.Bl == 1:
            noise = sh.par.gather_cfg(noise)                          # both halves of this frame shard
        if table:
            ops.cfg_euler_step_dev_(lat, noise, scal, self.g0, self.g1)
        else:
            ops.cfg_euler_step_(lat, noise, sigma, sigma_next, self.g0, self.g1)
        if self.round16:
            ops.cast_f16_to_f32(ops.cast_f32_to_f16(lat), out=lat)


class FlowControlNetPipeline:
    def __init__(self, vae=None, image_encoder=None, unet=None, controlnet=None, scheduler=None,
                 feature_extractor=None, parallel=None, round_latents_to_fp16=False, max_temporal_frames: int = MAX_TEMPORAL_FRAMES,
                 temporal_window=None, temporal_stream: bool = False):
        """parallel: optional ``parallel.FrameParallel`` -- this process then computes one CFG half / one frame shard
        of every clip (mofa_video_amd/parallel.py); all ranks must call the pipeline with identical inputs.
        round_latents_to_fp16: round the latents to fp16 after every Euler step, as the reference's fp16 run does.
        max_temporal_frames: the most frames one forward pass may hold (``num_frames``, or ``window_size`` of the window
        loop), 1 .. 128, or up to 256 under a ``temporal_window`` of radius <= 32 and anchor <= 32 (the temporal attention of
        more than 128 frames is mofa_attn_temporal_stream_local_f16; nothing at full geometry has been run above 128 frames).
        temporal_stream: True lifts that rule: up to 256 under ANY valid ``temporal_window``, None (dense) included.  Above 128
        frames dense attention and windows of radius > 32 or anchor > 32 then run through mofa_attn_temporal_stream_f16 (an
        online-softmax walk over the visible key tiles); everything else launches what it launches without the keyword.
        Nothing at full geometry has been run above 128 frames, and the memory of such a pass was not examined.
        Above the default of 32 the temporal attention runs through mofa_attn_temporal_long_f16; clips
        sharded over ranks (``parallel``) stay limited to 32 unless the parallel object was built with ``max_key_slots=`` (up
        to 128): then to the smaller of the two.  A sharded clip of more than 128 frames (up to the 256 admitted above) needs a
        parallel object built with ``stream_keys=True`` and, dense, ``max_key_slots`` at least the clip's frames: a rank's
        attention over more than 128 key slots then runs through mofa_attn_temporal_stream_shard_f16.  That path was run on
        one GPU only (virtual ranks, small geometry, and a rank's call alone at level-0 geometry); nothing ran on more than one
        GPU, no sharded clip of more than 128 frames ran at full geometry, and memory was not examined.
        temporal_window: None (dense temporal attention, the default: today's launches), an integer radius, or (radius,
        anchor): local temporal attention in every temporal layer of the UNet and the adapters -- query frame i sees key
        frame j iff j < anchor or |i - j| <= radius (mofa_attn_temporal_long_local_f16); an integer means (radius, 1), frame 0
        being the conditioning frame.  In the Keypoint window loop the rule applies inside every window (a window is one
        forward pass of window_size frames).  With a ``parallel`` object that shards frames it needs one built with
        ``window_keys=True``: every rank then exchanges ``radius`` frames with its neighbour shards and takes the anchor frames
        from shard 0 instead of gathering the clip, and attends through mofa_attn_temporal_long_window_f16.  The key slots of a
        rank, anchor + largest shard + 2 radius <= 128, then take the place of ``max_key_slots`` (``FrameParallel.window_plan``
        names the rule a layout breaks; a parallel object built with ``stream_keys=True`` as well takes up to 1024 slots, through
        mofa_attn_temporal_stream_shard_f16 above 128); ``max_temporal_frames`` still caps the frames of a forward pass.  That path has been
        checked over gloo on the CPU and on virtual ranks on one GPU; nothing was run on more than one GPU.  Nothing is
        claimed about what the released checkpoints produce under a window."""
        self.temporal_window = _temporal_window(temporal_window)
        if not isinstance(temporal_stream, bool):
            raise ValueError(f"temporal_stream must be True or False, got {temporal_stream!r}")
        self.temporal_stream = temporal_stream
        streams = temporal_stream or (self.temporal_window is not None and self.temporal_window[0] <= STREAM_RADIUS
                                      and self.temporal_window[1] <= STREAM_ANCHOR)
        if isinstance(max_temporal_frames, bool) or not isinstance(max_temporal_frames, int) \
                or not 1 <= max_temporal_frames <= (MAX_TEMPORAL_FRAMES_STREAM if streams else MAX_TEMPORAL_FRAMES_LONG):
            if temporal_stream:
                raise ValueError(f"max_temporal_frames must be an integer in 1 .. {MAX_TEMPORAL_FRAMES_STREAM} with "
                                 f"temporal_stream=True, got {max_temporal_frames!r}")
            raise ValueError(f"max_temporal_frames must be an integer in 1 .. {MAX_TEMPORAL_FRAMES_LONG}, or up to "
                             f"{MAX_TEMPORAL_FRAMES_STREAM} with temporal_window=(radius <= {STREAM_RADIUS}, anchor <= "
                             f"{STREAM_ANCHOR}), got {max_temporal_frames!r} with temporal_window={temporal_window!r}"
                             f" (temporal_stream=True: up to {MAX_TEMPORAL_FRAMES_STREAM} under any window, none included)")
        self.max_temporal_frames = max_temporal_frames
        self.vae, self.image_encoder, self.unet, self.controlnet = vae, image_encoder, unet, controlnet
        self.scheduler, self.feature_extractor = scheduler, feature_extractor
        self.vae_scale_factor = 8
        self.device = unet.device
        self.parallel = parallel
        self.round_latents_to_fp16 = round_latents_to_fp16
        self.overlap_adapter = True          # adapter trunk(s) || UNet encoder on two HIP streams (see _denoise_forward)
        self.split_decoder = True            # ... and the UNet decoder's two CFG halves on the same two streams
        # capture ONE denoise step per clip in a hipGraph and replay it for the remaining steps (no host scalar enters a step:
        # the scheduler's numbers come from a device table, _clip_loop).  Off for a rank that exchanges data inside a step (the
        # gloo / virtual-rank transports are host side), with a step callback, and while launches are being timed.
        self.graph_steps = GRAPH_STEPS_DEFAULT
        self._adapter_stream = None
        self._loop_stream = None

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, unet=None, controlnet=None, device="cuda", variant=None,
                        **modules):
        """the call of MOFA-Video-Traj/run_gradio.py:112-116: ``vae/``, ``image_encoder/`` (and ``unet/`` when not given) of
        a Stable-Video-Diffusion checkpoint directory; ``unet`` / ``controlnet`` (``face_controlnet`` / ``drag_controlnet``
        for the Hybrid class) are passed in already built, as the reference does.  Other diffusers keyword arguments
        (``torch_dtype``, ``low_cpu_mem_usage``, ``local_files_only`` ...) are accepted and ignored."""
        from .clip import CLIPVisionModelWithProjection
        from .scheduler import EulerDiscreteScheduler
        from .unet import UNetSpatioTemporalConditionControlNetModel
        from .vae import AutoencoderKLTemporalDecoder
        from . import checkpoint
        root = pretrained_model_name_or_path
        if unet is None:
            unet = UNetSpatioTemporalConditionControlNetModel.from_pretrained(root, subfolder="unet", device=device, variant=variant)
        vae = AutoencoderKLTemporalDecoder.from_pretrained(root, subfolder="vae", device=device, variant=variant)
        enc = CLIPVisionModelWithProjection.from_pretrained(root, subfolder="image_encoder", device=device, variant=variant)
        try:
            sch = EulerDiscreteScheduler(**{k: v for k, v in checkpoint.load_config(checkpoint.resolve_dir(root, "scheduler")).items()
                                            if k in EulerDiscreteScheduler().config})
        except OSError:
            sch = EulerDiscreteScheduler()
        names = ("face_controlnet", "drag_controlnet", "parallel", "round_latents_to_fp16", "feature_extractor", "max_temporal_frames",
                 "temporal_window", "temporal_stream")
        kw = {k: v for k, v in modules.items() if k in names}
        if controlnet is not None:
            kw["controlnet"] = controlnet
        return cls(vae=vae, image_encoder=enc, unet=unet, scheduler=sch, **kw)

    # ---- one network evaluation of a denoise step ---------------------------------------------------------------------------
    def _trunk_layers(self, adapters, masks, x_loc, t, emb, added_time_ids, Bl, Tl, half, fpar, h, w):
        """every adapter's ControlNet trunk, one after the other, then the blend of their residuals: a layer generator
        (``drive`` runs it through; blocks.run_lockstep interleaves it with the UNet's encoder) -> (12 residuals, mid residual)"""
        res = []
        for net, ctx, cond, scale in adapters:
            net.make_ctx(t, emb, added_time_ids, Bl, Tl, base=ctx, half=half, par=fpar, local=self.temporal_window)
            res.append((yield from net.forward_layers(x_loc, ctx, h, w, cond, scale)))
        down, mid = res[0]
        if len(res) == 2:
            down, mid = _blend_residuals(down, mid, res[1][0], res[1][1], masks, Bl * Tl)
        return down, mid

    def _encoder_layers(self, x_loc, t, emb, added_time_ids, Bl, Tl, half, fpar, h, w, c_un):
        self.unet.make_ctx(t, emb, added_time_ids, Bl, Tl, base=c_un, half=half, par=fpar, local=self.temporal_window)
        return (yield from self.unet.encode_layers(x_loc, c_un, h, w))

    def _denoise_forward(self, x_loc, t, emb, added_time_ids, Bl, Tl, half, fpar, h, w, adapters, c_un, masks=None):
        """``adapters``: [(controlnet, its Ctx, its per-clip condition, conditioning scale)], one entry, or two (face, drag)
        whose residuals are blended by ``masks`` (Hybrid/pipeline/pipeline.py:479-489) -> the UNet's noise prediction (tokens).
        Without frame sharding the trunks run on ``self._adapter_stream`` while the UNet's encoder half runs on the caller's
        stream; the streams join before the residuals are added (unet.decode_tokens).  Frame-sharded ranks enqueue the two
        networks layer by layer in lockstep so that their exchanges are issued in program order."""
        unet = self.unet
        net_args = (x_loc, t, emb, added_time_ids, Bl, Tl, half, fpar, h, w)
        trunks = self._trunk_layers(adapters, masks, *net_args)
        if not self.overlap_adapter or (fpar is not None and not fpar.two_streams):
            down, mid = drive(trunks)
            unet.make_ctx(t, emb, added_time_ids, Bl, Tl, base=c_un, half=half, par=fpar, local=self.temporal_window)
            return unet.forward_tokens(x_loc, c_un, h, w, down, mid)
        cur = torch.cuda.current_stream(self.device)
        if self._adapter_stream is None:
            self._adapter_stream = torch.cuda.Stream(device=self.device)
        side = self._adapter_stream
        side.wait_stream(cur)                                   # the model input (and everything before it) is ready
        if fpar is None:
            with torch.cuda.stream(side):
                down, mid = drive(trunks)
            unet.make_ctx(t, emb, added_time_ids, Bl, Tl, base=c_un, half=half, par=fpar, local=self.temporal_window)
            enc = unet.encode_tokens(x_loc, c_un, h, w)
        else:
            # Frame-sharded ranks: trunk(s) and UNet encoder still overlap on two HIP streams, but both issue collectives, and all
            # ranks must issue them in one order.  ONE host thread therefore enqueues both networks layer by layer in lockstep
            # (blocks.run_lockstep: a trunk layer on the second stream, the matching encoder layer on the caller's, ...): the order
            # is the program order on every rank, each network's wait for its GroupNorm partials / halo frames / token gather is a
            # stream wait covered by the other network's kernels, and the host never blocks (a second host thread under a turn
            # token gave the same order at 2.3 x the host time per step, profiles/r04_shard_proxy.log).  The decoder half runs on
            # the caller's stream alone.
            @contextlib.contextmanager
            def on_side():
                fpar.lane = 0
                with torch.cuda.stream(side):
                    yield

            @contextlib.contextmanager
            def on_cur():
                fpar.lane = 1
                yield
            try:
                (down, mid), enc = run_lockstep([trunks, self._encoder_layers(*net_args, c_un)], [on_side, on_cur])
            finally:
                fpar.lane = 0
        cur.wait_stream(side)
        for r in list(down) + [mid]:                            # allocated on the side stream, consumed (and freed) on this one
            r.record_stream(cur)
        if fpar is not None or not (self.split_decoder and Bl == 2 and half is None):
            return unet.decode_tokens(enc, c_un, down, mid)
        # The UNet's decoder half has nothing to run beside, so its two CFG halves go down the two streams (rows [0, rows) and
        # [rows, 2 rows) of every token tensor; the per-half contexts are the ones a rank of the 2-way CFG layout uses): one
        # half's GroupNorm / attention / epilogue phases overlap the other's MFMA phases.  Half-size launches choose their
        # tiles for themselves, so this order is deterministic but not bit-identical to the single-stream one.
        if c_un.halves is None:
            c_un.halves = [Ctx(1, Tl), Ctx(1, Tl)]
        sample, skips, counts, Hm, Wm = enc
        outs = [None, None]
        side.wait_stream(cur)                                   # the encoder's outputs are ready
        # Lifetime: the second half READS rows of `sample`, every skip and every residual on `side` while this function's
        # references may be dropped on `cur` (decode_tokens pops the skip views): tell the allocator about the second reader, so
        # that none of these blocks can be handed out again before `side` is done with them, whatever decode_tokens keeps alive
        for tt in [sample, mid] + list(skips) + list(down):
            tt.record_stream(side)
        for hf, st in enumerate((cur, side)):
            with torch.cuda.stream(st):
                ch = c_un.halves[hf]
                unet.make_ctx(t[hf:hf + 1] if torch.is_tensor(t) else t, emb, added_time_ids, 1, Tl, base=ch, half=hf, par=None,
                              local=self.temporal_window)
                outs[hf] = unet.decode_tokens((_rows_of(sample, hf), [_rows_of(k, hf) for k in skips], counts, Hm, Wm), ch,
                                              [_rows_of(r, hf) for r in down], _rows_of(mid, hf))
        cur.wait_stream(side)
        outs[1].record_stream(cur)
        return torch.cat(outs, 0)

    # ---- pieces of the reference __call__ ---------------------------------------------------------------------------------
    def check_inputs(self, image, height, width):                      # pipeline.py:222-234
        if image is not None and not torch.is_tensor(image) and not isinstance(image, list) and not hasattr(image, "convert"):
            raise ValueError("`image` has to be of type `torch.FloatTensor` or `PIL.Image.Image` or "
                             f"`List[PIL.Image.Image]` but is {type(image)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")

    def _check_call(self, batch_size, num_videos_per_prompt, max_guidance_scale, frames_per_forward):
        """The reference repeats the image embeddings / latents by ``num_videos_per_prompt`` (pipeline.py:130-131, :162) and draws
        ``batch_size * num_videos_per_prompt`` latents (:377-387), but doubles ``controlnet_condition`` / ``controlnet_flow`` only for
        CFG (:392-396) and builds ``added_time_ids`` for ``batch_size`` (:430-440): with anything but 1 x 1 its own
        ``FlowControlNet.forward`` / ``add_embedding`` reshape fail on the batch mismatch, and every entry point calls it with
        1 x 1.  One clip per call therefore IS the reference's behaviour; several videos = several calls with different
        generators / latents."""
        if batch_size != 1 or num_videos_per_prompt != 1:
            raise ValueError("one clip per call (batch_size = num_videos_per_prompt = 1, the only combination the reference's "
                             "own forward accepts: its controlnet_condition / added_time_ids are not repeated)")
        if not max_guidance_scale > 1.0:
            raise ValueError("the reference pipeline is only well-defined with classifier-free guidance on")
        windowed_shards = False
        if self.temporal_window is not None:
            if _shards_frames(self.parallel):
                if not getattr(self.parallel, "window_keys", False):
                    raise ValueError("temporal_window=... with a parallel object that shards frames: the gathered-key path of "
                                     "frame-sharded clips has no per-query mask (a CFG split alone and WindowParallel are fine)")
                windowed_shards = True          # built with window_keys=True: band + anchor keys, checked below
            if self.temporal_window[1] > frames_per_forward:
                raise ValueError(f"temporal_window anchor {self.temporal_window[1]} exceeds the {frames_per_forward} frames of a "
                                 "forward pass")
        limit = self.max_temporal_frames
        if frames_per_forward > limit:
            raise ValueError(f"{frames_per_forward} frames per forward pass: the temporal attention kernel handles at most "
                             f"{limit} (use KeypointFlowControlNetPipeline's window loop for long clips"
                             + (f", or build the pipeline with max_temporal_frames=... up to {MAX_TEMPORAL_FRAMES_LONG})"
                                if limit < MAX_TEMPORAL_FRAMES_LONG else ")"))
        if windowed_shards:
            # the key slots of a rank (anchor + largest shard + 2 radius <= 128) replace max_key_slots; window_plan names the
            # rule a layout breaks.  The same verdict on every rank: the rules read the layout alone
            fpar = getattr(self.parallel, "frame", self.parallel)
            if fpar.lay.T != frames_per_forward:
                raise ValueError(f"{frames_per_forward} frames per forward pass, but the parallel object's layout shards {fpar.lay.T}")
            try:
                fpar.window_plan(*self.temporal_window)
            except ValueError as e:             # past 128 key slots: name the keyword that lifts the limit (to 1024)
                if getattr(fpar, "stream_keys", False) or "exceed the attention kernel's 128" not in str(e):
                    raise
                raise ValueError(f"{e} (a parallel object built with stream_keys=True takes up to 1024 key slots)") from None
        elif self.parallel is not None:
            slots = getattr(self.parallel, "max_key_slots", MAX_TEMPORAL_FRAMES)
            if frames_per_forward > slots and slots == MAX_TEMPORAL_FRAMES:
                raise ValueError(f"{frames_per_forward} frames per forward pass with parallel=...: clips sharded over ranks are limited "
                                 f"to {MAX_TEMPORAL_FRAMES} frames (their gathered keys carry a 32-bit mask); run long clips on one device")
            if frames_per_forward > slots:
                hint = ""
                if frames_per_forward > MAX_TEMPORAL_FRAMES_LONG and not getattr(self.parallel, "stream_keys", False):
                    hint = (f" (more than {MAX_TEMPORAL_FRAMES_LONG} frames: build it with stream_keys=True and max_key_slots >= "
                            f"{frames_per_forward})")
                raise ValueError(f"{frames_per_forward} frames per forward pass with parallel=...: this parallel object takes clips of "
                                 f"at most max_key_slots = {slots} frames" + hint)

    def prepare_latents(self, batch_size, num_frames, num_channels_latents, height, width, generator, latents=None):
        shape = (batch_size, num_frames, num_channels_latents // 2, height // 8, width // 8)
        if latents is None:
            latents = torch.randn(shape, generator=generator, dtype=torch.float32,
                                  device=generator.device if generator is not None else "cpu")
        return latents.to(self.device, torch.float32) * self.scheduler.init_noise_sigma   # :272

    def _encode_image(self, image01):                                   # pipeline.py:114-139
        if self.image_encoder is None:
            raise ValueError("no image_encoder: pass image_embeddings=... or build the pipeline with one")
        return frontend.encode_image(self.image_encoder, image01)

    def _encode_vae_image(self, image01, noise_aug_strength, generator):  # pipeline.py:141-162, :338-352
        if self.vae is None or getattr(self.vae, "encoder", None) is None:
            raise ValueError("the VAE has no encoder weights: pass image_latents=... or load encoder.* / quant_conv.*")
        return frontend.encode_vae_image(self.vae, image01, noise_aug_strength, generator)

    def _conditioning(self, image, image_embeddings, image_latents, height=None, width=None, noise_aug_strength=0.02,
                      generator=None):
        """image: PIL / tensor in [0, 1] (what the reference's numpy_to_pt yields); either half can be supplied
        precomputed through the ``image_embeddings`` / ``image_latents`` extensions.  As in the reference the CLIP branch
        sees the image at its OWN size (pipeline.py:118-122: straight into the 224 x 224 antialiased resize), the VAE branch
        the ``preprocess(image, height, width)`` result (:338)."""
        dev = self.device
        if (image_embeddings is None or image_latents is None) and image is None:
            raise ValueError("pass `image`, or both image_embeddings=... and image_latents=...")
        if image_embeddings is None:
            image_embeddings = self._encode_image(frontend.image_to_01(image, None, None, dev))
        if image_latents is None:
            image_latents = self._encode_vae_image(frontend.image_to_01(image, height, width, dev), noise_aug_strength, generator)
        emb = image_embeddings.to(dev, torch.float32).reshape(-1, 1, image_embeddings.shape[-1])
        if emb.shape[0] == 1:                                             # :133-139 uncond = zeros
            emb = torch.cat([torch.zeros_like(emb), emb])
        il = image_latents.to(dev, torch.float32)
        if il.shape[0] == 1:                                              # :153-159
            il = torch.cat([torch.zeros_like(il), il])
        return emb, il.contiguous()

    def _condition_image(self, controlnet_condition, height, width):
        """``self.image_processor.preprocess(controlnet_condition, height=height, width=width)`` (pipeline.py:391): PIL /
        numpy / tensor, resized, [0, 1] -> [-1, 1] unless the tensor already holds negative values"""
        if controlnet_condition is None:
            raise ValueError("`controlnet_condition` is required")
        return frontend.preprocess(controlnet_condition, height, width, self.device)

    def _round(self, lat):
        if not self.round_latents_to_fp16:
            return lat
        return ops.cast_f16_to_f32(ops.cast_f32_to_f16(lat.contiguous())).reshape(lat.shape)


    def _clip_loop(self, lat, step, adapters, c_un, callback):
        """The denoise loop of one clip (pipeline.py:447-511) on this rank's CFG half / frames: ``lat`` fp32 [Tl,4,h,w] is stepped
        in place through every timestep of the scheduler and returned.

        Everything a step takes from the scheduler (sigma, sigma_next, the network's timestep, 1 / sqrt(sigma^2 + 1)) is uploaded
        ONCE per clip as a device table (scheduler.step_table) and the kernels read their row of it: no host scalar, no H2D copy
        inside a step.  That makes a step capturable: with ``graph_steps`` the first step runs eagerly (allocations, one-time
        kernel set-up, per-clip caches), the second is captured in a hipGraph on the loop's own stream -- its first node copies
        row ``counter`` of the table into a fixed ``cur`` row and increments the counter, every other node reads ``cur`` -- and
        steps 1 .. n-1 are replays: the host issues one graph launch per step instead of ~1 400 kernel launches."""
        sch, dev, sh = self.scheduler, self.device, step.sh
        n = len(sch.timesteps)
        self._num_timesteps = n
        tab = torch.from_numpy(sch.step_table()).to(dev)
        if not (self.graph_steps and callback is None and sh.par is None and ops.TIMER is None and n >= 3):
            for i, t in enumerate(sch.timesteps):
                step(lat, tab[i], adapters, c_un)
                if callback is not None:
                    new = self._callback(callback, i, t, lat, (1, sh.Tl, 4, step.h, step.w))
                    if new is not lat:
                        lat.copy_(new)
            return lat
        caller = torch.cuda.current_stream(dev)
        if self._loop_stream is None:
            self._loop_stream = torch.cuda.Stream(device=dev)
        gs = self._loop_stream
        gs.wait_stream(caller)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        cur = torch.empty(ops.STEP_SCALARS, dtype=torch.float32, device=dev)
        with torch.cuda.stream(gs):
            ops.step_select(tab, counter, cur)
            step(lat, cur, adapters, c_un)                                # step 0, eager
            graph = torch.cuda.CUDAGraph()
            graph.capture_begin()
            try:
                ops.step_select(tab, counter, cur)
                step(lat, cur, adapters, c_un)                            # (recorded, not executed)
            finally:
                graph.capture_end()
            for _ in range(1, n):
                graph.replay()
        caller.wait_stream(gs)
        lat.record_stream(gs)
        self._last_graph = graph                                          # keeps the graph's memory pool until the next clip
        return lat

    def _callback(self, cb, i, t, lat, shape):
        """callback_on_step_end(self, i, t, {"latents": ...}) may return replacement latents (pipeline.py:503-508)"""
        if cb is None:
            return lat
        out = cb(self, i, t, {"latents": lat.reshape(shape)})
        if out and "latents" in out:
            lat = out["latents"].to(self.device, torch.float32).reshape(lat.shape).contiguous()
        return lat

    def _decode(self, latents, T, decode_chunk_size, output_type, world, rank, owner=None, stream_chunks=None):
        """decode_latents + tensor2vid (pipeline.py:513-518).  With several ranks the independent VAE chunks (:204-213) are
        dealt round-robin (or as ``owner`` says: {chunk index: rank}): the result is then the list of (first_frame, frames)
        chunks this rank decoded.  stream_chunks: {chunk index: raw fp32 [n,3,H,W]} already decoded on a side stream (Keypoint
        loop)."""
        if output_type == "latent":
            return latents
        if world == 1 and not stream_chunks:
            frames = decode_latents(self.vae, latents, T, decode_chunk_size)           # fp32 [1,3,T,H,W]
            return frames if output_type == "raw" else tensor2vid(frames, None, output_type=output_type)
        stream_chunks = stream_chunks or {}
        sf = 1.0 / self.vae.config.scaling_factor
        chunks = []
        for ci, s0 in enumerate(range(0, T, decode_chunk_size)):
            if (owner[ci] if owner else ci % world) != rank:
                continue
            z = latents[0, s0:s0 + decode_chunk_size]
            fr = stream_chunks[ci] if ci in stream_chunks else self.vae.decode(z, num_frames=z.shape[0], _prescale=sf)   # fp32 [n,3,H,W]
            if world > 1 and output_type != "raw":
                fr = tensor2vid(fr.permute(1, 0, 2, 3).unsqueeze(0), None, output_type=output_type)[0]
            chunks.append((s0, fr))
        if world > 1:
            return chunks
        fr = torch.cat([fr for _, fr in chunks], 0)
        frames = fr.reshape(-1, T, *fr.shape[1:]).permute(0, 2, 1, 3, 4).float()
        return frames if output_type == "raw" else tensor2vid(frames, None, output_type=output_type)

    # ---- what the three __call__s share -------------------------------------------------------------------------------------
    def _prologue(self, image, height, width, num_frames, frames_per_forward, decode_chunk_size, batch_size, num_videos_per_prompt,
                  max_guidance_scale, num_inference_steps, noise_aug_strength, generator, latents, image_embeddings, image_latents,
                  controlnet_condition, more_checks=None):
        """Steps 1 .. 5 of the reference ``__call__`` in its order (pipeline.py:313-397): defaults, input checks (``more_checks``:
        the calling class's own, after the common ones), image conditioning (computed before the hot path), schedule, initial
        latents (every rank prepares the full clip's and keeps its own frames later) and the adapter's condition image (identical
        for both CFG halves, :393-397 -> computed once) -> (T, decode_chunk_size, h, w, emb, il, lat fp32 [T,4,h,w], cond)"""
        T = num_frames if num_frames is not None else self.unet.config.num_frames
        decode_chunk_size = decode_chunk_size if decode_chunk_size is not None else T
        self.check_inputs(image, height, width)
        self._check_call(batch_size, num_videos_per_prompt, max_guidance_scale, frames_per_forward if frames_per_forward is not None else T)
        if more_checks is not None:
            more_checks(T)
        h, w = height // 8, width // 8
        emb, il = self._conditioning(image, image_embeddings, image_latents, height, width, noise_aug_strength, generator)
        self.scheduler.set_timesteps(num_inference_steps)
        lat = self.prepare_latents(1, T, self.unet.config.in_channels, height, width, generator, latents).reshape(T, 4, h, w).contiguous()
        cond = self._condition_image(controlnet_condition, height, width)
        return T, decode_chunk_size, h, w, emb, il, lat, cond

    def _run_clip(self, sh, lat, il, emb, networks, masks, h, w, gmin, gmax, callback):
        """Denoise one clip on this rank's shard ``sh`` of it (2-way CFG x frame shards) and reassemble the
        clip's latents on every rank.  lat: the whole clip's fp32 [T,4,h,w]; networks: [(adapter, its ``prepare_condition`` for
        the frames (sh.f0, sh.f1), its conditioning scale)], two of them with the ``masks`` that blend their residuals."""
        lat = lat[sh.f0:sh.f1].contiguous()
        g0, g1 = sh.guidance(gmin, gmax)
        step = _Step(self, sh, il, emb, [net for net, _, _ in networks], masks, h, w, g0, g1, self.round_latents_to_fp16)
        adapters = [(net, Ctx(sh.Bl, sh.Tl), cond, scale) for net, cond, scale in networks]   # the Ctxs hold the per-clip caches
        lat = self._clip_loop(lat, step, adapters, Ctx(sh.Bl, sh.Tl), callback)                # :447-511
        return sh.gather(lat, h, w)

    def _epilogue(self, lat, decode_chunk_size, output_type, return_dict, controlnet_flow, world, rank, owner=None, stream_chunks=None):
        """lat: the clip's final latents [T,4,h,w] -> what ``__call__`` returns (pipeline.py:513-527)"""
        T = lat.shape[0]
        frames = self._decode(lat.reshape(1, T, *lat.shape[1:]), T, decode_chunk_size, output_type, world, rank, owner, stream_chunks)
        if not return_dict:
            return frames, controlnet_flow
        return FlowControlNetPipelineOutput(frames=frames, controlnet_flow=controlnet_flow)

    # ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, image=None, controlnet_condition=None, controlnet_flow=None, height: int = 576,
                 width: int = 1024, num_frames: Optional[int] = None, num_inference_steps: int = 25,
                 min_guidance_scale: float = 1.0, max_guidance_scale: float = 3.0, fps: int = 7,
                 motion_bucket_id: int = 127, noise_aug_strength: float = 0.02,
                 decode_chunk_size: Optional[int] = None, num_videos_per_prompt: Optional[int] = 1,
                 generator=None, latents: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                 callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], return_dict: bool = True,
                 controlnet_cond_scale=1.0, batch_size=1, *, image_embeddings=None, image_latents=None):
        T, decode_chunk_size, h, w, emb, il, lat, cond = self._prologue(
            image, height, width, num_frames, None, decode_chunk_size, batch_size, num_videos_per_prompt, max_guidance_scale,
            num_inference_steps, noise_aug_strength, generator, latents, image_embeddings, image_latents, controlnet_condition)
        flow = controlnet_flow.to(self.device, torch.float32)
        sh = _Shard(self.parallel, T)
        warped = self.controlnet.prepare_condition(cond[:1], flow[:1], frames=(sh.f0, sh.f1))
        lat = self._run_clip(sh, lat, il, emb, [(self.controlnet, warped, controlnet_cond_scale)], None, h, w,
                             min_guidance_scale, max_guidance_scale, callback_on_step_end)
        return self._epilogue(lat, decode_chunk_size, output_type, return_dict, controlnet_flow, sh.world, sh.rank)


# =========================================================================================================
# Hybrid: face (landmark) adapter + drag (trajectory) adapter, residuals blended by the user mask
# (MOFA-Video-Hybrid/pipeline/pipeline.py:293-320 signature, :443-507 loop, :479-489 blend)
# =========================================================================================================
def _resized_masks(mask, height, width, h, w, dev):
    """user mask [1,1,H,W] nearest-resized to the four residual resolutions (:481, :488); timestep-invariant"""
    m = mask.to(dev, torch.float32).reshape(1, height, width)
    masks, hh, ww = {}, h, w
    for _ in range(4):
        masks[hh * ww] = ops.resize_nearest_f32(m, hh, ww).reshape(-1).contiguous()
        hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    return masks


def _blend_residuals(df, mf, dd, md, masks, nframes):
    """face * m + drag * (1 - m) on all 12 + 1 residuals (:479-489)"""
    down = []
    for a, b in zip(df, dd):
        hw = a.shape[0] // nframes
        down.append(ops.mask_blend(a, b, masks[hw], hw))
    hw = mf.shape[0] // nframes
    return down, ops.mask_blend(mf, md, masks[hw], hw)



class HybridFlowControlNetPipeline(FlowControlNetPipeline):
    def __init__(self, vae=None, image_encoder=None, unet=None, face_controlnet=None, drag_controlnet=None,
                 scheduler=None, feature_extractor=None, parallel=None, round_latents_to_fp16=False,
                 max_temporal_frames: int = MAX_TEMPORAL_FRAMES, temporal_window=None, temporal_stream: bool = False):
        super().__init__(vae, image_encoder, unet, face_controlnet, scheduler, feature_extractor, parallel=parallel,
                         round_latents_to_fp16=round_latents_to_fp16, max_temporal_frames=max_temporal_frames,
                         temporal_window=temporal_window, temporal_stream=temporal_stream)
        self.face_controlnet, self.drag_controlnet = face_controlnet, drag_controlnet

    @torch.no_grad()
    def __call__(self, image=None, controlnet_condition=None, controlnet_flow=None, landmarks=None, drag_flow=None,
                 mask=None, height: int = 576, width: int = 1024, num_frames: Optional[int] = None,
                 num_inference_steps: int = 25, min_guidance_scale: float = 1.0, max_guidance_scale: float = 3.0,
                 fps: int = 7, motion_bucket_id: int = 127, noise_aug_strength: float = 0.02,
                 decode_chunk_size: Optional[int] = None, num_videos_per_prompt: Optional[int] = 1, generator=None,
                 latents: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                 callback_on_step_end=None, callback_on_step_end_tensor_inputs: List[str] = ["latents"],
                 return_dict: bool = True, ctrl_scale_traj=1.0, ctrl_scale_ldmk=1.0, batch_size=1, *,
                 image_embeddings=None, image_latents=None):
        face, drag, dev = self.face_controlnet, self.drag_controlnet, self.device
        T, decode_chunk_size, h, w, emb, il, lat, cond = self._prologue(
            image, height, width, num_frames, None, decode_chunk_size, batch_size, num_videos_per_prompt, max_guidance_scale,
            num_inference_steps, noise_aug_strength, generator, latents, image_embeddings, image_latents, controlnet_condition)
        sh = _Shard(self.parallel, T)
        fr = (sh.f0, sh.f1)
        cf = face.prepare_condition(cond[:1], controlnet_flow.to(dev, torch.float32)[:1], landmarks[:1], frames=fr)
        cd = drag.prepare_condition(cond[:1], drag_flow.to(dev, torch.float32)[:1], frames=fr)
        masks = _resized_masks(mask, height, width, h, w, dev)
        lat = self._run_clip(sh, lat, il, emb, [(face, cf, ctrl_scale_ldmk), (drag, cd, ctrl_scale_traj)], masks, h, w,
                             min_guidance_scale, max_guidance_scale, callback_on_step_end)
        return self._epilogue(lat, decode_chunk_size, output_type, return_dict, controlnet_flow, sh.world, sh.rank)


# =========================================================================================================
# Keypoint long video ("periodic sampling"): overlapping temporal windows with frame 0 prepended, one Euler step per
# window, overlap average (MOFA-Video-Keypoint/pipeline/svdxt_pipeline_ctrlnet_loop.py:289-294 signature,
# :426-429 views, :445-511 loop)
# =========================================================================================================
def _deal_ready_chunks(ready, world, busy_next, idle_cap=3, busy_cap=2):
    """Which rank decodes the VAE chunks that became final before the last round(s) of the last denoise step: a rank with no
    window in the next round takes up to ``idle_cap`` of them (a chunk decode is about a third of a window step), a rank that
    is stepping a window up to ``busy_cap`` on its second stream (a window finalises 1.5 chunks per round at stride 12 and
    chunks of 8); the rest wait for the next round.  Pure function of its arguments: every rank computes the same table."""
    idle = [r for r in range(world) if r not in busy_next]
    slots = [r for k in range(idle_cap) for r in idle] + [r for k in range(busy_cap) for r in busy_next]
    return list(zip(ready, slots))


def window_views(num_frames, window_size, stride):
    window_num = (num_frames - window_size) // stride + 1
    views = [(1 + i * stride, i * stride + window_size) for i in range(window_num)]
    return views + [(num_frames - window_size + 1, num_frames)]


WindowLayout = collections.namedtuple("WindowLayout", "framepar wpar world rank nslots slot")


def window_layout(parallel, window_size):
    """Several windows, four ways to spread them (the pipeline's ``parallel``; parallel.window_layout_costs prices them):
      None            every window on this GPU, one after the other;
      WindowParallel  the distinct windows of a step dealt to the ranks, one all-gather per round;
      FrameParallel   (Layout of window_size frames) every window on ALL ranks, 2-way CFG x frame shards inside the
                      window, the stepped window gathered before the overlap average -- the layout for more ranks than
                      windows (on 8 ranks and 7 windows WindowParallel's single round is the faster of the two);
      GroupedWindowParallel  G groups of g ranks: windows dealt to the groups, frame-parallel inside a group.
    In all of them every rank holds all N latent frames and applies the same overlap average in view order.
    -> framepar: what shards the frames of a window, or None; wpar: what deals the windows, or None; world, rank: over which
    ranks the VAE chunks are dealt; nslots, slot: the windows of a round and which of them this rank steps."""
    from .parallel import FrameParallel, GroupedWindowParallel
    grouped = parallel if isinstance(parallel, GroupedWindowParallel) else None
    framepar = parallel if isinstance(parallel, FrameParallel) else (grouped.frame if grouped is not None else None)
    wpar = grouped if grouped is not None else (parallel if framepar is None else None)
    if wpar is not None:                                              # (world, rank global: VAE chunks go to all ranks)
        return WindowLayout(framepar, wpar, wpar.world, wpar.rank, len(wpar.rounds([None])[0]), wpar.slot)
    sh = _Shard(framepar, window_size)
    return WindowLayout(framepar, None, sh.world, sh.rank, 1, 0)


class WindowPlan:
    """The overlap average of one denoise step over ``views`` (svdxt_pipeline_ctrlnet_loop.py:502-511) as tables, no tensors:
    ``value[0:t1] += window`` for the first view, ``value[t0:t1] += window[1:]`` for the others, in view order, then
    ``latents = value / count``.  ``count[f]`` = the views that cover frame f (a repeated view counts again)."""

    def __init__(self, views, num_frames, decode_chunk_size):
        if views[0][0] != 1:
            raise ValueError("the first window must start at frame 1")
        self.views, self.N, self.chunk = list(views), num_frames, decode_chunk_size
        self.nchunks = -(-num_frames // decode_chunk_size)
        self.count, self.last_view_of, self.adds = [0] * num_frames, [-1] * num_frames, []
        for idx, (t0, t1) in enumerate(self.views):
            dst0, src0 = (0, 0) if idx == 0 else (t0, 1)
            self.adds.append([(idx, src0 + k, dst0 + k, self.count[dst0 + k] == 0) for k in range(t1 - dst0)])
            for f in range(dst0, t1):
                self.count[f] += 1
                self.last_view_of[f] = idx            # the last covering view in processing order: f is final once it is merged

    def accumulations(self, m, since=0):
        """what merging the views [since, m) issues, in order: (view, row of its window, frame, first touch of that frame?)"""
        return [a for adds in self.adds[since:m] for a in adds]

    def frontier(self, m):
        """with the views [0, m) merged the frames [0, frontier) are final: their last covering view is among them"""
        f = 0
        while f < self.N and self.last_view_of[f] < m:
            f += 1
        return f

    def ready_chunks(self, m):
        """the decode chunks that lie wholly below ``frontier(m)``"""
        F = self.frontier(m)
        return [ci for ci in range(self.nchunks) if min((ci + 1) * self.chunk, self.N) <= F]


class _WindowLoop:
    """One call of the window loop: the stepped windows of a timestep are averaged into ``lat`` fp32 [N,4,h,w] as ``plan`` says.
    windows: {view: (its adapters, its UNet Ctx)} of the DISTINCT views, in view order; step: the ``_Step`` of a window."""

    def __init__(self, pipe, lo, views, plan, step, windows, lat, overlap_decode):
        self.pipe, self.lo, self.views, self.plan, self.step, self.windows, self.lat = pipe, lo, views, plan, step, windows, lat
        self.value = torch.empty_like(lat)
        self.rounds = lo.wpar.rounds(list(windows)) if lo.wpar is not None else [[k] for k in windows]
        # the decode of finished frames overlaps the rest of the LAST step on a second HIP stream wherever that step has more
        # than one round; a chunk belongs to ``owner[ci]`` (the same table on every rank)
        self.side = torch.cuda.Stream(device=pipe.device) if (overlap_decode and len(self.rounds) > 1) else None
        self.stream_chunks, self.owner = {}, {}

    def step_window(self, lat_in, view, scal):
        """-> the window ``view`` of ``lat_in`` after one step, all its frames [Tw,4,h,w]"""
        sh = self.step.sh
        lw = torch.cat([lat_in[0:1], lat_in[view[0]:view[1]]], dim=0)             # frame 0 + window frames
        lw = lw[sh.f0:sh.f1].contiguous()                                         # (this rank's frames of the window)
        self.step(lw, scal, *self.windows[view])
        return sh.gather(lw, self.step.h, self.step.w)

    def step_round(self, lat_in, rnd, scal, done):
        wpar = self.lo.wpar
        if wpar is None:
            done[rnd[0]] = self.step_window(lat_in, rnd[0], scal)
            return
        mine = rnd[self.lo.slot]                                  # window-parallel: one window per rank and round
        lw = self.step_window(lat_in, mine, scal) if mine is not None else \
            torch.zeros((self.step.sh.T,) + tuple(self.lat.shape[1:]), dtype=self.lat.dtype, device=self.lat.device)
        for key, got in zip(rnd, wpar.gather(lw)):
            if key is not None:
                done[key] = got

    def merge(self, m0, m1, done):
        """value[0:t1] += lw (first view) / value[t0:t1] += lw[1:] (others)   (:502-507)"""
        for idx, src, f, first in self.plan.accumulations(m1, since=m0):
            ops.axpby_f32_(done[self.views[idx]][src].reshape(-1), self.value[f].reshape(-1), 1.0, 0.0 if first else 1.0)

    def finalize(self, frames):
        """latents = where(count > 0, value / count, value) (:511; value is 0 where no window landed)"""
        for f in frames:
            if self.plan.count[f]:
                ops.axpby_f32_(self.value[f].reshape(-1), self.lat[f].reshape(-1), 1.0 / self.plan.count[f], 0.0)
            else:
                self.lat[f].zero_()

    def decode_on_side(self, chunks):
        """the VAE decode of the (final) frames of ``chunks`` on the second stream, behind everything enqueued so far"""
        vae, n, lat_r = self.pipe.vae, self.plan.chunk, self.pipe._round(self.lat)
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            lat_r.record_stream(self.side)                        # (lat_r may be a temporary of the main stream: keep its
            for ci in chunks:                                     #  block out of the allocator until the decode ran)
                z = lat_r[ci * n:min(ci * n + n, self.plan.N)]
                self.stream_chunks[ci] = vae.decode(z, num_frames=z.shape[0], _prescale=1.0 / vae.config.scaling_factor)

    def deal_ready(self, merged, next_round):
        """-> the chunks that became final with the views [0, merged) and are this rank's to decode while ``next_round`` runs"""
        lo = self.lo
        ready = [ci for ci in self.plan.ready_chunks(merged) if ci not in self.owner]
        busy_next = [r for r in range(lo.world) if lo.wpar is None or next_round[r * lo.nslots // lo.world] is not None]
        for ci, r in _deal_ready_chunks(ready, lo.world, busy_next):
            self.owner[ci] = r
        return [ci for ci in ready if self.owner.get(ci) == lo.rank]

    def run_step(self, scal, overlap):
        views, plan, done = self.views, self.plan, {}
        # every window of a step reads the latents of the PREVIOUS step; when frames are finalised while later windows
        # of the (last) step still run, those windows read a snapshot
        lat_in = self.lat.clone() if overlap else self.lat
        merged, frontier = 0, 0                               # views [0, merged) are merged, frames [0, frontier) final
        for ri, rnd in enumerate(self.rounds):
            self.step_round(lat_in, rnd, scal, done)
            if not overlap or ri == len(self.rounds) - 1:
                continue
            # views are merged in view order as soon as their window is stepped (the same summation order as after the
            # loop); every frame whose last covering view is merged can be averaged now, and whole decode chunks below
            # the frontier go to the second stream while the next round runs
            m = merged
            while m < len(views) and views[m] in done:
                m += 1
            self.merge(merged, m, done)
            newf = plan.frontier(m)
            self.finalize(range(frontier, newf))
            merged, frontier = m, newf
            mine = self.deal_ready(merged, self.rounds[ri + 1])
            if mine:
                self.decode_on_side(mine)
        self.merge(merged, len(views), done)
        self.finalize(range(frontier, plan.N))

    def run(self, callback):
        """every timestep of the scheduler -> (latents, {chunk: its rank}, {chunk: frames already decoded})"""
        pipe, sch = self.pipe, self.pipe.scheduler
        n = pipe._num_timesteps = len(sch.timesteps)
        for i, t in enumerate(sch.timesteps):
            self.run_step((t, *sch.sigma_pair(i)), overlap=(i == n - 1 and self.side is not None))
            self.lat = pipe._callback(callback, i, t, pipe._round(self.lat), (1,) + tuple(self.lat.shape))
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)
            if callback is not None:
                self.stream_chunks, self.owner = {}, {}   # a callback may have replaced the latents after the last step
        rest = [ci for ci in range(self.plan.nchunks) if ci not in self.owner]   # the chunks still to decode: dealt evenly
        for j, ci in enumerate(rest):
            self.owner[ci] = j % self.lo.world
        return self.lat, self.owner, self.stream_chunks


class KeypointFlowControlNetPipeline(FlowControlNetPipeline):
    """The window loop of the reference's long-video pipeline.  Two extensions beyond it (new work, BASELINE config 5):
    * hybrid control inside the windows: built with a ``drag_controlnet`` and called with ``drag_flow`` / ``mask``, every
      window runs the landmark adapter AND the trajectory adapter and blends their residuals by the mask, exactly as
      ``HybridFlowControlNetPipeline`` does per clip (Hybrid/pipeline/pipeline.py:479-489);
    * the VAE decode overlaps the last denoise step: in that step the windows finish in order, so every decode chunk whose
      frames are final is decoded on a second HIP stream while the remaining windows are still being stepped.  With several
      ranks the same holds per round (``parallel.WindowParallel``: a round = one window per rank; ranks without a window in
      the next round take the finished chunks first) or per window (``parallel.FrameParallel``: every window on all ranks),
      and the chunks not decoded early are dealt evenly after the loop."""

    def __init__(self, vae=None, image_encoder=None, unet=None, controlnet=None, scheduler=None, feature_extractor=None,
                 parallel=None, round_latents_to_fp16=False, drag_controlnet=None, overlap_decode=True,
                 max_temporal_frames: int = MAX_TEMPORAL_FRAMES, temporal_window=None, temporal_stream: bool = False):
        super().__init__(vae, image_encoder, unet, controlnet, scheduler, feature_extractor, parallel=parallel,
                         round_latents_to_fp16=round_latents_to_fp16, max_temporal_frames=max_temporal_frames,
                         temporal_window=temporal_window, temporal_stream=temporal_stream)
        self.drag_controlnet = drag_controlnet
        self.overlap_decode = overlap_decode

    def _check_windows(self, Tw, stride, hybrid, mask, N):
        if N < Tw:
            raise ValueError(f"num_frames ({N}) must be at least window_size ({Tw})")
        if not 0 < stride < Tw:
            raise ValueError(f"stride ({stride}) must lie in (0, window_size = {Tw}): consecutive windows have to overlap")
        if hybrid and (self.drag_controlnet is None or mask is None):
            raise ValueError("hybrid control needs a drag_controlnet (constructor) and a mask")

    @torch.no_grad()
    def __call__(self, image=None, controlnet_condition=None, controlnet_flow=None, landmarks=None, window_size: int = 25,
                 stride: int = 12, height: int = 576, width: int = 1024, num_frames: Optional[int] = None,
                 num_inference_steps: int = 25, min_guidance_scale: float = 1.0, max_guidance_scale: float = 3.0,
                 fps: int = 7, motion_bucket_id: int = 127, noise_aug_strength: float = 0.02,
                 decode_chunk_size: Optional[int] = None, num_videos_per_prompt: Optional[int] = 1, generator=None,
                 latents: Optional[torch.FloatTensor] = None, output_type: Optional[str] = "pil",
                 callback_on_step_end=None, callback_on_step_end_tensor_inputs: List[str] = ["latents"],
                 return_dict: bool = True, controlnet_cond_scale=1.0, batch_size=1, *, image_embeddings=None,
                 image_latents=None, drag_flow=None, mask=None, ctrl_scale_traj=1.0):
        cn, drag, dev = self.controlnet, self.drag_controlnet, self.device
        Tw, hybrid = window_size, drag_flow is not None
        N, decode_chunk_size, h, w, emb, il, lat, cond = self._prologue(
            image, height, width, num_frames, Tw, decode_chunk_size, batch_size, num_videos_per_prompt, max_guidance_scale,
            num_inference_steps, noise_aug_strength, generator, latents, image_embeddings, image_latents, controlnet_condition,
            more_checks=functools.partial(self._check_windows, Tw, stride, hybrid, mask))
        flow = controlnet_flow.to(dev, torch.float32)
        dflow = drag_flow.to(dev, torch.float32) if hybrid else None
        masks = _resized_masks(mask, height, width, h, w, dev) if hybrid else None
        views = window_views(N, Tw, stride)
        lo = window_layout(self.parallel, Tw)
        sh = _Shard(lo.framepar, Tw)
        fr = dict(frames=(sh.f0, sh.f1)) if lo.framepar is not None else {}
        if lo.framepar is not None and lo.wpar is None and len(set(views)) == 1 and N == Tw:
            # ONE window that is the whole clip (N == window_size: every view is frames 1 .. N-1 behind frame 0): the loop
            # degenerates to the plain denoise loop -- value = k * stepped window, count = k -- so the clip is frame-sharded
            # exactly like FlowControlNetPipeline / HybridFlowControlNetPipeline (2-way CFG x frame shards) and the latents
            # stay sharded between the steps.
            # window = frame 0 + frames 1 .. N-1 with the flows of frames 1 .. N-1 (svdxt_pipeline_ctrlnet_loop.py:470-476)
            networks = [(cn, cn.prepare_condition(cond[:1], flow[:1, 0:N - 1], landmarks[:, 0:N], **fr), controlnet_cond_scale)]
            if hybrid:
                networks.append((drag, drag.prepare_condition(cond[:1], dflow[:1, 0:N - 1], **fr), ctrl_scale_traj))
            lat = self._run_clip(sh, lat, il, emb, networks, masks, h, w, min_guidance_scale, max_guidance_scale, callback_on_step_end)
            return self._epilogue(lat, decode_chunk_size, output_type, return_dict, controlnet_flow, sh.world, sh.rank)
        # adapter state per DISTINCT window is timestep-invariant: computed once per clip (the reference recomputes it
        # every step; its last view often repeats the previous one -- SURVEY 3.5 -- and is computed once here)
        windows = {}
        for (t0, t1) in views:
            if (t0, t1) in windows:
                continue
            lm = torch.cat([landmarks[:, 0:1], landmarks[:, t0:t1]], dim=1)
            adapters = [(cn, Ctx(sh.Bl, sh.Tl), cn.prepare_condition(cond[:1], flow[:1, t0 - 1:t1 - 1], lm, **fr), controlnet_cond_scale)]
            if hybrid:
                adapters.append((drag, Ctx(sh.Bl, sh.Tl), drag.prepare_condition(cond[:1], dflow[:1, t0 - 1:t1 - 1], **fr), ctrl_scale_traj))
            windows[(t0, t1)] = (adapters, Ctx(sh.Bl, sh.Tl))
        gmin, gmax = min_guidance_scale, max_guidance_scale
        g0, g1 = sh.guidance(gmin, gmax) if lo.framepar is not None else (gmin, gmax)   # of this rank's frames of a window
        step = _Step(self, sh, il, emb, [cn] + ([drag] if hybrid else []), masks, h, w, g0, g1)
        loop = _WindowLoop(self, lo, views, WindowPlan(views, N, decode_chunk_size), step, windows, lat,
                           self.overlap_decode and output_type != "latent")
        lat, owner, stream_chunks = loop.run(callback_on_step_end)
        return self._epilogue(lat, decode_chunk_size, output_type, return_dict, controlnet_flow, lo.world, lo.rank, owner, stream_chunks)
