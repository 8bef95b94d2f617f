"""process() and its helpers with the reference's names and argument meaning (test_scripts/inference.py:39-166,
scripts/DMD/transformer_train/generate.py:22-87), running on the HIP path.

When the four models are instarevive_amd objects sharing one context, process() issues ONE call through the C ABI
(ir_pipeline): uint8 HWC in, uint8 HWC out, everything in between stays on the GPU in NHWC bf16 / fp32 statistics.
The stage-by-stage form (the reference's literal sequence of Python calls) is kept for drop-in use and for tests.
"""
import ctypes as C
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .models import AutoencoderKL, ControlTransformerHalf, DDPMScheduler, SwinIR, Transformer2DModel, prompt_bias


class _Staging:
    """Host <-> device staging of one image batch shape: page-locked host buffers (so the 12.6 MB per 2048 x 2048 image cross PCIe
    by DMA at link rate instead of through a pageable bounce copy) and the matching device buffers, kept per shape on the context.
    `slots` independent sets let process_stream() upload batch i+1 and download batch i-1 while batch i computes."""

    def __init__(self, device, n, h, w, slots=1):
        shape = (n, h, w, 3)
        self.shape = shape
        self.h_in = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.h_out = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.h_st1 = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.d_in = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(slots)]
        self.d_out = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(slots)]
        self.d_st1 = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(slots)]
        self.h2d_done = [None] * slots   # event behind the last asynchronous upload out of h_in[slot] (see upload())

    @staticmethod
    def get(ctx, n, h, w, slots=1, tag="sync"):
        pool = ctx.__dict__.setdefault("_staging", {})
        key = (tag, n, h, w, slots)
        if key not in pool:
            if len(pool) >= 8:  # bounded: drop the oldest shape
                pool.pop(next(iter(pool)))
            pool[key] = _Staging(ctx.device, n, h, w, slots)
        return pool[key]

    def fill(self, slot, control_imgs):
        """Copy the caller's HWC uint8 arrays into the pinned input buffer of `slot` (one pass, no intermediate np.stack)."""
        if self.h2d_done[slot] is not None:   # the previous upload out of this pinned buffer may still be queued behind earlier kernels
            self.h2d_done[slot].synchronize()
            self.h2d_done[slot] = None
        dst = self.h_in[slot].numpy()
        for i, im in enumerate(control_imgs):
            if im.dtype != np.uint8 or im.shape != self.shape[1:]:
                raise ValueError("control_imgs must be HWC uint8 RGB arrays of equal size")
            np.copyto(dst[i], im)

    def upload(self, slot, stream=None):
        """Asynchronous H2D copy of the pinned input buffer of `slot` on `stream` (default: the current one). The event recorded behind
        it is what the next fill() of the slot waits for: a caller that never synchronises with the device between two images (a
        rank that only contributes tiles under --shard_tiles) must not overwrite the pinned buffer while its copy is still queued."""
        self.d_in[slot].copy_(self.h_in[slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream(self.d_in[slot].device))
        self.h2d_done[slot] = ev
        return ev


def _png_encoder(ctx, count, h, w, slot=0, tag="sync", runs=False):
    """The PngEncoder (png.py) of a batch shape and staging slot, kept on the context like the staging buffers. Each entry holds count x ir_png_bound
    bytes on the device and as much page-locked host memory (about 14 MB per 2048 x 2048 image; twice the images with stage-1 output, two slots
    under process_stream). At most 8 entries: the oldest is dropped whatever its use, which is safe because a batch in flight keeps its own
    reference (_Batch.enc), and costs a re-allocation when more than 8 shapes alternate. runs: the encoder's run mode (ir_png_encode_runs), part
    of the key: the two modes never share an entry."""
    from .png import PngEncoder
    pool = ctx.__dict__.setdefault("_png", {})
    key = (tag, count, h, w, slot, bool(runs))
    if key not in pool:
        if len(pool) >= 8:
            pool.pop(next(iter(pool)))
        pool[key] = PngEncoder(ctx, count, h, w, runs)
    return pool[key]


def _jpeg_encoder(ctx, codec, count, h, w, slot=0, tag="sync"):
    """The JpegEncoder (jpeg.py) of a batch shape, (quality, subsampling) and staging slot, pooled on the context like the PNG encoders (a pool of
    its own, at most 8 entries). Each entry holds count x ir_jpeg_bound bytes on the device and as much page-locked host memory: the bound is the
    worst case of any pixels at any quality, about 41 MB per 2048 x 2048 image in 4:2:0, of which a photograph at quality 95 fills 1 - 2 MB."""
    from .jpeg import JpegEncoder
    pool = ctx.__dict__.setdefault("_jpeg", {})
    key = (tag, count, h, w, slot) + tuple(codec)
    if key not in pool:
        if len(pool) >= 8:
            pool.pop(next(iter(pool)))
        pool[key] = JpegEncoder(ctx, count, h, w, codec[0], codec[1])
    return pool[key]


def _jpeg_codec(png, jpeg, quality, subsampling):
    """(quality, subsampling in PIL's numbers) of a call with jpeg=, None of one without; jpeg= and png= exclude each other."""
    if jpeg is None:
        return None
    if png is not None:
        raise ValueError("jpeg= and png= exclude each other: a result is saved in one format")
    from .jpeg import check_params, subsampling_of
    codec = (int(quality), subsampling_of(subsampling))
    check_params(*codec)
    return codec


def _check_images(control_imgs):
    if len(control_imgs) == 0:
        raise ValueError("control_imgs is empty")
    first = np.asarray(control_imgs[0])
    if first.dtype != np.uint8 or first.ndim != 3 or first.shape[-1] != 3:
        raise ValueError("control_imgs must be HWC uint8 RGB arrays")
    return len(control_imgs), first.shape[0], first.shape[1]


def _sliding_windows(h: int, w: int, tile_size: int, tile_stride: int):
    hi_list = list(range(0, h - tile_size + 1, tile_stride))
    if (h - tile_size) % tile_stride != 0:
        hi_list.append(h - tile_size)
    wi_list = list(range(0, w - tile_size + 1, tile_stride))
    if (w - tile_size) % tile_stride != 0:
        wi_list.append(w - tile_size)
    return [(hi, hi + tile_size, wi, wi + tile_size) for hi in hi_list for wi in wi_list]


def eps_to_mu(scheduler, model_output, sample, timesteps):
    acp = scheduler.alphas_cumprod.to(device=sample.device, dtype=sample.dtype)
    a = acp[timesteps]
    while a.ndim < sample.ndim:
        a = a.unsqueeze(-1)
    return (sample - (1 - a) ** 0.5 * model_output) / a ** 0.5


def forward_model(model, latents, timestep, prompt_embeds, prompt_attention_masks=None, c=None):
    added = {"resolution": None, "aspect_ratio": None}
    if model.config.sample_size == 128:   # generate.py:56-62: micro-conditioning on the latent's height / width
        bsz, _, height, width = latents.shape
        added = {"resolution": torch.tensor([height, width]).repeat(bsz, 1).to(prompt_embeds.dtype),
                 "aspect_ratio": torch.tensor([float(height / width)]).repeat(bsz, 1).to(prompt_embeds.dtype)}
    timestep = timestep.expand(latents.shape[0])
    if c is None:
        noise_pred = model(latents, timestep=timestep, encoder_hidden_states=prompt_embeds, encoder_attention_mask=prompt_attention_masks,
                           added_cond_kwargs=added).sample
    else:  # ControlTransformerHalf returns the tensor itself (generate.py:74-82)
        noise_pred = model(latents, timestep=timestep, encoder_hidden_states=prompt_embeds, encoder_attention_mask=prompt_attention_masks,
                           added_cond_kwargs=added, c=c)
    if model.config.out_channels // 2 == latents.shape[1]:
        noise_pred = noise_pred.chunk(2, dim=1)[0]
    return noise_pred


def generate_sample_1step(model, scheduler, latents, maxt, prompt_embeds, prompt_attention_masks=None, c=None):
    if isinstance(model, Transformer2DModel) and c is None:  # fused epilogue: eps half + eps_to_mu inside the HIP path
        return model.step(latents, float(maxt), float(scheduler.alphas_cumprod[int(maxt)]), prompt_embeds, prompt_attention_masks)
    if isinstance(model, ControlTransformerHalf) and c is not None:
        return model.step(latents, float(maxt), float(scheduler.alphas_cumprod[int(maxt)]), prompt_embeds, prompt_attention_masks, c=c)
    t = torch.full((1,), maxt, device=latents.device).long()
    noise_pred = forward_model(model, latents=latents, timestep=t, prompt_embeds=prompt_embeds, prompt_attention_masks=prompt_attention_masks, c=c)
    return eps_to_mu(scheduler, noise_pred, latents, t)


def wavelet_reconstruction(content_feat, style_feat):
    return _color_fix(L.FLAG_FIX_WAVELET, content_feat, style_feat)


def adaptive_instance_normalization(content_feat, style_feat):
    return _color_fix(L.FLAG_FIX_ADAIN, content_feat, style_feat)


def _color_fix(kind, content, style):
    from .models import get_context
    ctx = get_context(content.device)
    content = content.to(torch.float32).contiguous()
    style = style.to(content.device, torch.float32).contiguous()
    n, ch, h, w = content.shape
    if ch != 3 or style.shape != content.shape:
        raise ValueError("colour fix expects two [B,3,H,W] tensors of equal shape")
    out = torch.empty_like(content)
    ws = ctx.workspace(ctx.ws_bytes(L.STAGE_COLORFIX, n, h, w))
    ctx.check(ctx.lib.ir_color_fix(ctx.h, ctx.stream(), kind, L.ptr(content), L.ptr(style), L.ptr(out), n, h, w, L.ptr(ws), ws.numel()),
              "ir_color_fix")
    return out


def _fused_ok(model, preprocess_model, vae, disable_preprocess_model):
    if not (isinstance(model, (Transformer2DModel, ControlTransformerHalf)) and isinstance(vae, AutoencoderKL)):
        return False
    if not disable_preprocess_model and not isinstance(preprocess_model, SwinIR):
        return False
    ctxs = {id(m.ctx) for m in (model, vae) if m.ctx is not None}
    if not disable_preprocess_model and preprocess_model.ctx is not None:
        ctxs.add(id(preprocess_model.ctx))
    return len(ctxs) == 1


def _pipeline_flags(model, color_fix_type, disable_preprocess_model, tiled):
    flags = (L.FLAG_NO_PREPROCESS if disable_preprocess_model else 0) | (L.FLAG_TILED if tiled else 0)
    if tiled:
        flags |= {"wavelet": L.FLAG_FIX_WAVELET, "adain": L.FLAG_FIX_ADAIN}.get(color_fix_type, 0)
    if isinstance(model, ControlTransformerHalf):
        flags |= L.FLAG_CONTROL_LQ
    return flags


def _prepare_fused(model, y, y_mask, h, w, tiled, tile_size, others=(), set_prompt=True):
    for m in others:  # the context must hold THESE models' weights (another instance of the family may have been loaded since)
        if m is not None:
            m._ready()
    model._ready()    # a ControlTransformerHalf re-binds its control branch here (set_prompt below resolves to the base model only)
    if set_prompt:
        model.set_prompt(y, y_mask)
    if tiled:
        model.ensure_pos(tile_size // 16, tile_size // 16)
    else:
        model.ensure_pos(h // 16, w // 16)


def _launch_pipeline(ctx, st, slot, n, h, w, flags, tile_size, tile_stride, acp, sf, want_stage1=True):
    ws = ctx.workspace(ctx.ws_bytes(L.STAGE_PIPELINE, n, h, w, flags, tile_size, tile_stride))
    ctx.check(ctx.lib.ir_pipeline(ctx.h, ctx.stream(), L.ptr(st.d_in[slot]), L.ptr(st.d_out[slot]), L.ptr(st.d_st1[slot]) if want_stage1 else None,
                                  n, h, w, flags, tile_size, tile_stride, 400.0, acp, sf, L.ptr(ws), ws.numel()), "ir_pipeline")


class _Batch:
    """One batch in flight through the fused form: what it was given, the buffers it travels in (the staging set, the resample.ResizeSlot of a
    resize batch, the scorer slots, the PNG encoder) and one method per phase, in this order - plan (the constructor), upload, reserve, launch,
    download, collect. process() runs them on one stream with a wait in between; process_stream() overlaps the phases of neighbouring batches on
    two streams and keeps the batch's events in `ready` (its uploads) and `done` (its downloads)."""

    def __init__(self, ctx, slot, tag, slots, shape, imgs, with_stage1, rects=None, records=None, dparams=None, gts=None, lpips=False, niqe=None,
                 clipiqa=False, sizes=None, want_lq=False, prompts=(None, None), codec=None, png_runs=False, musiq=False, maniqa=False, dists=False, fid=None, fid_sizes=None, ilniqe=None, topiq=False):
        """The plan phase, host work only: every size is checked and every ground truth compared with its image's FINAL size, so a batch that
        does not fit raises ValueError before anything is launched for it; then the scorer slots are filled / planned - `scorers` holds them in
        the order of a score tuple: paired (metrics.ScoreSlot; with lpips it scores LPIPS as well, ir_lpips with the weights lpips.configure()
        bound to the context), NIQE with `niqe` its parameters, IL-NIQE with `ilniqe` its template (ilniqe.configure() bound to the context), CLIP-IQA, MUSIQ, MANIQA (maniqa: True, or the images' names, which key random crops), TOPIQ-NR (topiq.configure() bound to the context), and last DISTS (dists: ir_dists with the weights dists.configure() bound to the context; the paired slot queues it, metrics.DistsColumn
        stands where its value is read) - and the images copied into page-locked memory: the staging input, or
        the decoded files (with their degrade parameters) into the ResizeSlot, whose bicubic chain then makes the staging input on the device.
        fid: None, or FID's resize mode - the batch's predictions (and its ground truth, when it has one) go through ir_fid_features into a
        fid.FidSlot, which is no scorer: FID has no per-file value, so collect() hands the features over beside the scores; fid_sizes: the
        batch's fid_rects entry.
        sizes: the batch's niqe_rects entry. codec: None - rects are coded as PNG, in the run mode with png_runs - or _jpeg_codec()'s pair."""
        from .slots import final_sizes, record_sizes
        self.ctx, self.slot, self.tag, self.shape, self.with_stage1 = ctx, slot, tag, shape, with_stage1
        self.rects, self.records, self.dparams, self.prompts = rects, records, dparams, prompts
        self.want_lq = want_lq and dparams is not None
        self.codec, self.png_runs = codec, bool(png_runs)
        self.enc = self.ready = self.done = None
        n, h, w = shape
        copies = 2 if with_stage1 else 1
        self.sc, self.scorers = None, []
        if gts is not None:
            from .metrics import ScoreSlot
            gts, min_edge = list(gts), None   # every image needs 11 x 11 pixels for SSIM's window, 31 x 31 with LPIPS
            if lpips:
                from .lpips import MIN_EDGE, configured
                if not configured(ctx):
                    raise ValueError("lpips=True: no LPIPS weights are bound to the context (instarevive_amd.lpips.configure)")
                min_edge = MIN_EDGE
            final_sizes("gt", n, h, w, records, rects, gts=gts, min_edge=min_edge)
            self.sc = ScoreSlot.get(ctx, slot, tag)
            if dists:
                from .dists import configured as dists_configured
                if not dists_configured(ctx):
                    raise ValueError("dists=True: no DISTS weights are bound to the context (instarevive_amd.dists.configure)")
            self.sc.fill(gts, lpips, copies, dists=bool(dists))
            self.scorers.append(self.sc)
        if niqe is not None or ilniqe is not None or clipiqa or musiq or maniqa or topiq:
            finals = final_sizes("niqe" if niqe is not None else "ilniqe" if ilniqe is not None else "clipiqa" if clipiqa else "musiq" if musiq else "maniqa" if maniqa else "topiq", n, h, w, records, rects, sizes, gts)
            if niqe is not None:
                from .niqe import NiqeSlot
                self.scorers.append(NiqeSlot.get(ctx, slot, tag))
                self.scorers[-1].plan(finals, niqe, copies)
            if ilniqe is not None:
                from .ilniqe import IlniqeSlot, configured
                if not configured(ctx):
                    raise ValueError("ilniqe=...: IL-NIQE's tables are not bound to the context (instarevive_amd.ilniqe.configure)")
                self.scorers.append(IlniqeSlot.get(ctx, slot, tag))
                self.scorers[-1].plan(finals, ilniqe, copies)
            if clipiqa:
                from .clipiqa import ClipIqaSlot
                self.scorers.append(ClipIqaSlot.get(ctx, slot, tag))
                self.scorers[-1].plan(finals, copies)
            if musiq:
                from .musiq import MusiqSlot
                self.scorers.append(MusiqSlot.get(ctx, slot, tag))
                self.scorers[-1].plan(finals, copies)
            if maniqa:
                from .maniqa import ManiqaSlot
                self.scorers.append(ManiqaSlot.get(ctx, slot, tag))
                self.scorers[-1].plan(finals, copies, None if maniqa is True else list(maniqa))
            if topiq:
                from .topiq import TopiqSlot
                self.scorers.append(TopiqSlot.get(ctx, slot, tag))
                self.scorers[-1].plan(finals, copies)
        if gts is not None and dists:
            from .metrics import DistsColumn
            self.scorers.append(DistsColumn(self.sc))
        self.fid = None
        if fid:
            from .fid import FidSlot
            self.fid = FidSlot.get(ctx, slot, tag)
            self.fid.plan(final_sizes("fid", n, h, w, records, rects, fid_sizes, gts), fid, self.sc)
        if rects is not None:
            if records is None and len(rects) != n:
                raise ValueError(f"{'png' if codec is None else 'jpeg'}: {len(rects)} rectangles for a batch of {n} images")
            if records is not None and [tuple(r) for r in rects] != record_sizes(records):
                raise ValueError(f"{'png' if codec is None else 'jpeg'}: the rectangles {list(rects)} of a resize batch are not its final sizes {record_sizes(records)}")
        self.st = _Staging.get(ctx, n, h, w, slots=slots, tag=tag)
        self.rs = None
        if records is None:
            self.st.fill(slot, imgs)
        else:   # the decoded files travel; the network input is made on the device
            from .resample import ResizeSlot
            self.rs = ResizeSlot.get(ctx, slot, tag)
            self.rs.fill(records, dparams)

    def upload(self, stream=None, owner=None):
        """Asynchronous H2D copies of what plan staged - the images, then the ground truth - on `stream` (default: the current one), which the
        caller has made current; owner: the compute stream when it is another one (ResizeSlot.upload). Returns the event behind the last copy:
        the later event of one stream covers both uploads."""
        ev = self.st.upload(self.slot, stream) if self.rs is None else self.rs.upload(stream, owner)
        return ev if self.sc is None else self.sc.upload(stream, owner)

    def reserve(self):
        """Every growth of the context's workspace (and the scorers' own scratch) that the calls around the network need - the PNG encoder, the
        resampling calls ahead of and behind the network, the scorers - BEFORE the pipeline's launch takes the workspace's address: a recorded
        graph is keyed by it."""
        n, h, w = self.shape
        if self.rects is not None and self.codec is None:
            self.ctx.workspace(self.ctx.ws_bytes(L.STAGE_PNG_RUNS if self.png_runs else L.STAGE_PNG, n, h, w))
        elif self.rects is not None:
            from .jpeg import RESTART_MCUS
            self.ctx.workspace(self.ctx.ws_bytes(L.STAGE_JPEG, n, h, w, self.codec[1], RESTART_MCUS))
        if self.records is not None:
            from .resample import chain_ws_bytes, decode_ws_bytes
            self.ctx.workspace(max(chain_ws_bytes(self.records), decode_ws_bytes(self.records)))
        for s in self.scorers + ([self.fid] if self.fid is not None else []):
            s.reserve()

    def launch(self, flags, tile_size, tile_stride, acp, sf):
        """The batch's device work on the current stream: [ir_degrade of the decoded files] -> the bicubic chain into the staging input ->
        ir_pipeline -> LANCZOS of the valid rectangles back to the LQ sizes -> ir_png_encode / ir_jpeg_encode of every image's final form -> every scorer's calls.
        What stands behind ir_pipeline runs behind the replay of a recorded graph, outside the recording. `outs` lists the outputs the later
        phases walk: (first row, the network's output [n][h][w][3], per image its resized result [1][th][tw][3] or None for a plain crop - None
        for all without resize records), the predictions at rows 0 .. n - 1 and - with stage-1 output - the stage-1 images at n .. 2n - 1."""
        from .slots import record_sizes
        ctx, st, slot, rs, (n, h, w) = self.ctx, self.st, self.slot, self.rs, self.shape
        if rs is not None:
            rs.decode(self.records)   # the batch's JPEG and PNG files (JpegSource / PngSource records), into the places of their pixels
            if self.dparams is not None:
                rs.degrade(self.records)
            rs.to_network(self.records, st.d_in[slot])
        _launch_pipeline(ctx, st, slot, n, h, w, flags, tile_size, tile_stride, acp, sf, self.with_stage1)
        outs = [(0, st.d_out[slot])] + ([(n, st.d_st1[slot])] if self.with_stage1 else [])
        if rs is not None:
            rs.reserve_results(n, h, w, self.with_stage1)
        self.outs = [(first, out, rs.back_to_lq(self.records, out, first) if rs is not None else None) for first, out in outs]
        if self.rects is not None:   # the batch keeps its own reference to the encoder: the pool evicts after 8 shapes
            if self.codec is None:
                self.enc = _png_encoder(ctx, len(outs) * n, h, w, slot, self.tag, self.png_runs)
            else:
                self.enc = _jpeg_encoder(ctx, self.codec, len(outs) * n, h, w, slot, self.tag)
            for first, out, res in self.outs:
                if res is None:
                    self.enc.queue(first, out, self.rects)
                else:   # the resized result, or the valid rectangle of the network's output
                    for i, (r, final) in enumerate(zip(res, record_sizes(self.records))):
                        self.enc.queue(first + i, out[i:i + 1] if r is None else r, [final])
        for s in self.scorers + ([self.fid] if self.fid is not None else []):
            for first, out, res in self.outs:
                s.queue(first, out, res)

    def download(self):
        """The batch's D2H copies on the current stream, behind its device work: the byte counts of an encoded batch - the raw images are then
        not downloaded - else the network's output and / or the resized results (a batch whose results were all resized back downloads those
        alone); the LQ images of a degraded batch when a sink wants them; every scorer's rows."""
        st, slot = self.st, self.slot
        if self.enc is not None:
            self.enc.fetch_sizes()
        else:
            if self.rs is None or any(r is None for r in self.outs[0][2]):
                st.h_out[slot].copy_(st.d_out[slot], non_blocking=True)
                if self.with_stage1:
                    st.h_st1[slot].copy_(st.d_st1[slot], non_blocking=True)
            if self.rs is not None:
                self.rs.download([r for _, _, res in self.outs for r in res])
        if self.want_lq:
            self.rs.download_lq()
        if self.rs is not None:
            self.rs.download_info()
        for s in self.scorers + ([self.fid] if self.fid is not None else []):
            s.download()

    def host_lq(self):
        """The LQ images of a degraded batch (want_lq), after the downloads have completed."""
        return self.rs.host_lq(self.records)

    def collect(self, stream=None, png_wrap=True):
        """After the downloads have completed: process()'s result - (preds, stage1_preds) as arrays the caller owns (the pinned buffers are
        reused by the slot's next batch) or as PNG files, whose bytes are fetched here on `stream` now that their counts are known - and, for a
        scored batch, the scores element: a pair of lists (predictions, stage-1 images or empty) of tuples, every scorer's values in the order of
        `scorers`. The host part of NIQE (the fits and the score) runs here, where the scores are read."""
        n = self.shape[0]
        if self.rs is not None:
            self.rs.check_info(self.records)
        if self.enc is not None:
            files = self.enc.fetch(len(self.outs) * n, stream, png_wrap)
            lists = [files[:n], files[n:]]
        else:
            lists = []
            for (_, _, res), host in zip(self.outs, (self.st.h_out[self.slot], self.st.h_st1[self.slot])):
                if res is None:
                    host = host.clone().numpy()
                    lists.append([host[i] for i in range(n)])
                else:   # the resized result, or the valid rectangle of the network's output
                    host = host.numpy()
                    lists.append([self.rs.host_result(r) if r is not None else host[i, :rec.geo.valid_hw[0], :rec.geo.valid_hw[1]].copy()
                                  for i, (rec, r) in enumerate(zip(self.records, res))])
            lists.append([])
        fid = () if self.fid is None else (self.fid.features(),)   # the last element of a batch with fid: {"fid": [n][2048], "fid_gt": ... or None}
        if not self.scorers:
            return (lists[0], lists[1]) + fid
        scores = [[sum(row, ()) for row in zip(*(s.scores(first, n) for s in self.scorers))] for first, _, _ in self.outs] + [[]]
        return (lists[0], lists[1], (scores[0], scores[1])) + fid


def _batch_shape(imgs, records):
    """(n, h, w) of a batch: of its resize records' network input when it has them (the image list is then not read), else of its images."""
    if records is not None:
        from .resample import check_records
        return check_records(records)
    return _check_images(imgs)


@torch.no_grad()
def process(model, control_imgs: List[np.ndarray], strength: float, color_fix_type: str, disable_preprocess_model: bool, tiled: bool,
            tile_size: int, tile_stride: int, preprocess_model=None, vae=None, y=None, y_mask=None, noise_scheduler=None,
            fused: bool = True, graph: bool = False, return_stage1: bool = True, fp8: bool = False, png=None,
            resize=None, gt=None, lpips: bool = False, niqe=None, niqe_rects=None, clipiqa: bool = False, degrade=None,
            lq_sink=None, jpeg=None, jpeg_quality: int = 95, jpeg_subsampling=2, png_runs: bool = False, musiq: bool = False, maniqa=False, dists: bool = False, fid=None,
            fid_rects=None, ilniqe=None, topiq: bool = False) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """test_scripts/inference.py:55-166. control_imgs: list of HWC uint8 RGB arrays of equal size (multiples of 64).
    Returns (preds, stage1_preds) as lists of HWC uint8 arrays (stage1_preds is empty with return_stage1=False, which skips its
    conversion and download).

    Extension (no reference counterpart: the reference's process() never passes c): when `model` is a ControlTransformerHalf, the
    one-step call becomes generate_sample_1step(..., c=<the scaled LQ latent the step starts from>), per tile under `tiled`.
    graph=True (fused form only): the launch sequence is recorded into a hipGraph per image size / flag set and replayed on later
    calls. Images travel through page-locked staging buffers kept per batch shape (which also gives a recorded graph stable
    device addresses). fp8=True (fused form, BASELINE.json configs[4]): fp8 MFMA operands in the VAE resnet convolutions
    (vae.enable_fp8() must have uploaded the fp8 weight forms).
    png (fused form only): a list of one valid rectangle (vh, vw) per image. The results are then encoded on the GPU (ir_png_encode queued behind
    ir_pipeline - under graph=True behind the graph's replay, not inside the recording) and both lists hold PNG files as `bytes` of the
    top-left vh x vw crops instead of arrays; only the compressed bytes are downloaded. png_runs=True (with png): the encoder's run mode,
    ir_png_encode_runs - the same pixels, runs of equal filtered bytes coded as matches, no file larger than without it.
    jpeg (fused form only; exclusive with png): the same list of rectangles, and the lists hold baseline JPEG files instead - ir_jpeg_encode at
    jpeg_quality (1 .. 100) and jpeg_subsampling (2 or 420: 4:2:0, 0 or 444: 4:4:4), byte for byte PIL's Image.save(format="JPEG", quality,
    subsampling, restart_marker_blocks=jpeg.RESTART_MCUS) of the raw result. It combines with resize, degrade, gt, niqe and clipiqa as png does;
    the scores are those of the device's image, the result BEFORE the JPEG loss.
    resize (fused form only): a list of one resample.ResizeJob per image - the DECODED file (or a jpeg_decode.JpegSource / png_decode.PngSource: the file's
    compressed bytes are uploaded and ir_jpeg_decode / ir_png_decode makes the pixels on the device, Pillow's bytes; a stream the device cannot
    decode raises RuntimeError when the batch is collected) and its job_geometry(). control_imgs is then not read:
    the decoded bytes are uploaded, ir_resample_u8 makes the network input on the device (the bicubic chain of --sr_scale / auto_resize, the
    zero pad), and behind ir_pipeline the valid rectangle of every image that auto_resize enlarged is resampled (LANCZOS) back to its LQ size.
    Both lists then hold the FINAL images - what the command line saves: the resized result, else the valid rectangle - bit for bit what
    PIL gives around a plain call; with png their files (the rectangles are then the final sizes).
    A job whose geometry is resample.crop_geometry() is centre-cropped on the device instead (utils.center_crop_arr's BOX halvings and bicubic
    resize, the last step ir_resample_u8_window straight into the network input): its final image is the image_size x image_size prediction;
    the jobs of a batch may come from files of different sizes. With degrade the crop is made first and is what is degraded.
    gt (fused form only): a list of one ground-truth image per image, HWC uint8 RGB of the image's FINAL size (the png rectangle, the final size
    of a resize job, else any top-left rectangle of the network's output). ir_metrics_y is queued behind ir_pipeline (and the LANCZOS calls; under
    graph=True behind the replay) and the call returns a triple (preds, stage1_preds, scores): scores is a pair of lists of (psnr_y, ssim_y), for
    the predictions and - with return_stage1, else empty - the stage-1 images, by tools/evaluate_pairs.py's definitions. A ground truth of
    another size raises ValueError before anything is launched.
    lpips (with gt only): score LPIPS as well - ir_lpips with the weights instarevive_amd.lpips.configure() bound to the models' context, queued
    behind ir_metrics_y on the same images. Every score is then (psnr_y, ssim_y, lpips); every image needs at least 31 x 31 pixels.
    niqe (fused form only; with or without gt): the pristine parameters (mu_prisparam, cov_prisparam) of instarevive_amd.niqe.load_params().
    ir_niqe_stats is queued behind the network (and the paired scores) on every image's FINAL form - the png rectangle, the final size of a resize
    job, niqe_rects (one (h, w) per image), the ground truth's size, else the whole output - and the fits and the score are computed on the host
    when the scores are read. Alone, the call returns the triple with scores a pair of lists of (niqe,); with gt the value is appended to each
    tuple. An image without a score (an edge below 96 pixels, fewer than two complete feature rows) gets NaN.
    ilniqe (fused form only; with or without gt and the other scores): the template of instarevive_amd.ilniqe.load_params(), with
    instarevive_amd.ilniqe.configure() bound to the models' context. ir_ilniqe_stats is queued behind ir_niqe_stats on the same final forms
    (niqe_rects serves it too); its value stands right behind NIQE's in every tuple: (ilniqe,), (niqe, ilniqe), (psnr_y, ssim_y[, lpips][, niqe], ilniqe, ...).
    clipiqa (fused form only; with or without gt and niqe): score CLIP-IQA as well - ir_clipiqa with the model instarevive_amd.clipiqa.configure()
    bound to the models' context, queued behind ir_niqe_stats on the same final rectangles (niqe_rects serves both). Its value is the last of
    every tuple: (clipiqa,), (niqe, clipiqa), (psnr_y, ssim_y[, lpips][, niqe], clipiqa). An image below 32 pixels on an edge gets NaN.
    musiq (fused form only; alone or with gt, lpips, niqe and clipiqa): score MUSIQ as well - ir_musiq with the model instarevive_amd.musiq.configure()
    bound to the models' context, queued behind ir_clipiqa on the same final rectangles (niqe_rects serves it too). Its value comes behind
    clipiqa's, the last of every tuple. An image of which a resized side rounds to 0 (1 x 1000) gets NaN.
    maniqa (fused form only; alone or with the others): score MANIQA as well - ir_maniqa with the model instarevive_amd.maniqa.configure() bound to
    the models' context, queued behind ir_musiq on the same final rectangles. True, or one name per image: with maniqa.configure(mode="random")
    an image's crop origins are drawn from the seed and its name (its row in the batch without names). Its value is the last of every tuple.
    An image whose short side is not above the crop (224) gets NaN.
    topiq (fused form only; alone or with the others): score TOPIQ-NR as well - ir_topiq with the model instarevive_amd.topiq.configure() bound to
    the models' context, queued behind ir_maniqa on the same final rectangles. Its value comes behind maniqa's and before dists's in every
    tuple. An image with a side below 16 gets NaN.
    dists (with gt only): score DISTS as well - ir_dists with the weights instarevive_amd.dists.configure() bound to the models' context, queued
    behind ir_lpips on the same images. Its value is the very last of every tuple, behind maniqa's; a pair below 16 pixels on an edge gets NaN.
    fid (with or without gt): True / "clean" / "legacy" - the Inception-v3 features of FID (ir_fid_features with the weights
    instarevive_amd.fid.configure() bound to the models' context) of every prediction at its final size, queued behind the other scorers, and of
    the ground truth when gt= is given. FID is a statistic of a whole set, so there is no score column: the result gains a LAST element, the dict
    {"fid": [n][2048] float64, "fid_gt": [n][2048] or None}, which the caller collects (fid.FeatureSet) and scores at the end of the run
    (fid.frechet_distance). fid_rects: one (h, w) per image where the final size is neither a resize record's, a png rectangle nor the ground truth's.
    degrade (with resize): one instarevive_amd.degrade.Params (or one degrade.ChainParams - the second-order chain, ir_degrade_chain; a batch
    holds one kind) per image - the decoded files are GROUND TRUTH, and between the upload and the
    bicubic chain ir_degrade makes each one's LQ image on the device (blur, bilinear downsample, noise, JPEG round trip, bilinear resize back;
    tools/degrade_folder.py is the definition), which the network then restores. lq_sink: called once with the list of those LQ images (HWC
    uint8, the decoded files' sizes) after they have been downloaded, before process() returns."""
    noise_scheduler = noise_scheduler or DDPMScheduler()
    if lpips and gt is None:
        raise ValueError("process(lpips=True) needs gt=: LPIPS is scored against the ground truth")
    if dists and gt is None:
        raise ValueError("process(dists=True) needs gt=: DISTS is scored against the ground truth")
    if degrade is not None and resize is None:
        raise ValueError("process(degrade=...) needs resize=: the ground truth is degraded on the device input route")
    n, h, w = _batch_shape(control_imgs, resize)
    codec = _jpeg_codec(png, jpeg, jpeg_quality, jpeg_subsampling)
    if (png is not None or jpeg is not None or resize is not None or gt is not None or niqe is not None or ilniqe is not None or clipiqa or musiq or maniqa or topiq) and not (fused and _fused_ok(model, preprocess_model, vae, disable_preprocess_model)):
        raise ValueError("process(png=... / resize=... / gt=... / niqe=...) needs the fused form (instarevive_amd models sharing one context)")
    device = model.device
    acp = float(noise_scheduler.alphas_cumprod[400])
    sf = float(vae.config.scaling_factor)
    if fp8 and not (fused and _fused_ok(model, preprocess_model, vae, disable_preprocess_model)):
        raise ValueError("process(fp8=True) needs the fused form (instarevive_amd models sharing one context)")
    if fused and _fused_ok(model, preprocess_model, vae, disable_preprocess_model):
        if fp8 and not vae.__dict__.get("_fp8_uploaded"):
            raise RuntimeError("process(fp8=True): call vae.enable_fp8() first - without the fp8 weight forms every layer would silently run in bf16")
        ctx = model.ctx
        batch = _Batch(ctx, 0, "sync", 1, (n, h, w), control_imgs, return_stage1, png if codec is None else jpeg, resize, degrade, gt, lpips, niqe,
                       clipiqa, niqe_rects, lq_sink is not None, codec=codec, png_runs=png_runs, musiq=musiq, maniqa=maniqa, dists=dists,
                       fid=("clean" if fid is True else fid) or None, fid_sizes=fid_rects, ilniqe=ilniqe, topiq=bool(topiq))
        _prepare_fused(model, y, y_mask, h, w, tiled, tile_size, (vae, None if disable_preprocess_model else preprocess_model))
        flags = _pipeline_flags(model, color_fix_type, disable_preprocess_model, tiled) | (L.FLAG_GRAPH if graph else 0) | (L.FLAG_FP8 if fp8 else 0)
        batch.upload()
        batch.reserve()
        batch.launch(flags, tile_size, tile_stride, acp, sf)
        batch.download()
        torch.cuda.current_stream(device).synchronize()
        if batch.want_lq:
            lq_sink(batch.host_lq())
        return batch.collect()

    # ---- stage-by-stage form: the reference's literal call sequence on NCHW fp32 tensors
    if tiled:   # before any network runs: what ir_pipeline refuses with -31 (tile_geom in csrc/api.cpp)
        tl, sl = tile_size // 8, tile_stride // 8
        if tl <= 0 or sl <= 0 or sl > tl or tl > min(h, w) // 8 or tl % 2:
            raise ValueError(f"bad tile geometry for a {h}x{w} image: tile {tile_size}, stride {tile_stride}")
    imgs = np.ascontiguousarray(np.stack(control_imgs))
    control = torch.tensor(imgs / 255.0, dtype=torch.float32, device=device).clamp_(0, 1).permute(0, 3, 1, 2).contiguous()
    if not disable_preprocess_model:
        control = preprocess_model(control)
    height, width = control.shape[-2:]
    lh, lw = height // 8, width // 8
    c_latent = vae.encode(control * 2 - 1).latent_dist.mode().to(torch.float32)
    init_noise = c_latent * sf
    with_c = isinstance(model, ControlTransformerHalf)
    if not tiled:
        latents = generate_sample_1step(model, noise_scheduler, init_noise, 400, y, y_mask, c=init_noise if with_c else None)
        img_buffer = vae.decode(latents / sf).sample / 2 + 0.5
    else:
        wins = _sliding_windows(lh, lw, tl, sl)
        count = torch.zeros((n, 4, lh, lw), device=device)
        noise_buffer = torch.zeros_like(init_noise)
        for hi, he, wi, we in wins:
            tile = init_noise[:, :, hi:he, wi:we].contiguous()
            noise_buffer[:, :, hi:he, wi:we] += generate_sample_1step(model, noise_scheduler, tile, 400, y, y_mask, c=tile if with_c else None)
            count[:, :, hi:he, wi:we] += 1
        noise_buffer.div_(count)
        img_buffer = torch.zeros_like(control)
        count = torch.zeros_like(control)
        for hi, he, wi, we in wins:
            tile = vae.decode((noise_buffer[:, :, hi:he, wi:we] / sf).contiguous()).sample / 2 + 0.5
            cond = control[:, :, hi * 8:he * 8, wi * 8:we * 8].contiguous()
            if color_fix_type == "adain":
                tile = adaptive_instance_normalization(tile, cond)
            elif color_fix_type == "wavelet":
                tile = wavelet_reconstruction(tile, cond)
            img_buffer[:, :, hi * 8:he * 8, wi * 8:we * 8] += tile
            count[:, :, hi * 8:he * 8, wi * 8:we * 8] += 1
        img_buffer.div_(count)
    x_samples = (img_buffer.clamp(0, 1).permute(0, 2, 3, 1) * 255).cpu().numpy().clip(0, 255).astype(np.uint8)
    control = (control.permute(0, 2, 3, 1) * 255).cpu().numpy().clip(0, 255).astype(np.uint8)
    return [x_samples[i] for i in range(n)], [control[i] for i in range(n)]


def _split_batch(b):
    """A process_stream batch: a sequence of images, or an (images, y, y_mask) triple with the batch's own prompts (y a tensor)."""
    if isinstance(b, tuple) and len(b) == 3 and isinstance(b[1], torch.Tensor):
        return b[0], b[1], b[2]
    return b, None, None


@torch.no_grad()
def process_stream(model, batches: Iterable[Sequence[np.ndarray]], color_fix_type: str, disable_preprocess_model: bool, tiled: bool,
                   tile_size: int, tile_stride: int, preprocess_model=None, vae=None, y=None, y_mask=None, noise_scheduler=None,
                   return_stage1: bool = True, graph: bool = False, fp8: bool = False, png=None,
                   png_wrap: bool = True, resize=None, gt=None, lpips: bool = False, niqe=None,
                   niqe_rects=None, clipiqa: bool = False, degrade=None, lq_sink=None, jpeg=None, jpeg_quality: int = 95,
                   jpeg_subsampling=2, png_runs: bool = False, musiq: bool = False, maniqa=False, dists: bool = False, fid=None,
                   fid_rects=None, ilniqe=None, topiq: bool = False) -> Iterator[Tuple[List[np.ndarray], List[np.ndarray]]]:
    """process() over a sequence of image batches with the transfers hidden: while batch i computes on the current stream, batch
    i+1 is uploaded and batch i-1 downloaded on a copy stream (two staging slots per batch shape). Yields process()'s result for
    every batch, in order. Needs the fused form (all models instarevive_amd objects on one context). fp8 as in process() (cfg-5:
    vae.enable_fp8() first; the operand set is the context's ir_set_fp8_mask, by default the tolerance-chosen one).
    A batch may also be an (images, y, y_mask) triple: y [B, T, C] / y_mask (as set_prompt takes them) are that batch's prompts, one per image
    or one for all. They are queued on the stream right before the batch's launch (pinned upload, ir_dit_set_prompts: no host wait), so a
    recorded graph (graph=True) replays across batches whose prompts differ in content only. Batches without prompts take y / y_mask.
    png: an iterable in step with `batches` (it is advanced right after the batch is drawn, so a generator fed by the batch generator works): per
    batch None, or one valid rectangle (vh, vw) per image. For such a batch ir_png_encode is queued behind ir_pipeline on the compute stream for
    the predictions and, with return_stage1, the stage-1 images; under graph=True it runs behind the graph's replay and is not part of the
    recording. The copy stream then fetches the byte counts and only the produced bytes - the raw images are not downloaded - and the
    batch's two lists hold PNG files (`bytes`, the top-left vh x vw crops) in place of arrays. The chunk framing (one CRC-32 over the compressed
    bytes and their copy into the file, about 20 ms per 2048 x 2048 result) is done on the calling thread between launches; png_wrap=False yields
    (zlib stream, width, height) triples instead, for png.wrap_png(*triple) on a thread of the caller's (what inference.py's writer pool does).
    png_runs=True: every batch with png rectangles takes the encoder's run mode (ir_png_encode_runs), as in process().
    jpeg (exclusive with png): an iterable like png, and the files are JPEGs - ir_jpeg_encode at jpeg_quality / jpeg_subsampling, as in process().
    With png_wrap=False the lists hold (segment, width, height, quality, subsampling, restart_mcus) pieces for jpeg.wrap_jpeg(*pieces).
    resize: an iterable in step with `batches`, advanced like png: per batch None, or one resample.ResizeJob per image (the decoded file and its
    job_geometry(); images that reach one network size share a batch whatever their own sizes). The batch's image list is then not read. The copy
    stream uploads the decoded bytes, the compute stream runs ir_resample_u8 once or twice per image into the staging input ahead of ir_pipeline
    and, behind it, LANCZOS of the valid rectangles back to the LQ sizes where auto_resize enlarged; the batch's lists hold the final images
    as in process(resize=...), and with png (the rectangles are then the final sizes) every file of the batch comes from the device encoder.
    degrade: an iterable in step with `resize`, advanced like it: per batch None, or one instarevive_amd.degrade.Params (or degrade.ChainParams) per image - the decoded
    files are then ground truth and ir_degrade makes their LQ images on the device ahead of the bicubic chain, as in process(degrade=...); the
    kernels and noise fields ride the copy stream with the images. lq_sink: called with the list of a batch's LQ images (downloaded on the
    copy stream) right before that batch's results are yielded.
    gt: an iterable in step with `batches`, advanced like png / resize: per batch None, or one ground-truth image per image - HWC uint8 RGB of the
    image's FINAL size (the png rectangle, the final size of a resize job, else any top-left rectangle of the network's output). The copy stream
    uploads them with the batch, ir_metrics_y is queued behind ir_pipeline and the LANCZOS calls on the compute stream (under graph=True behind the
    replay, outside the recording) and the scores come back with the batch's download. Such a batch yields a triple (preds, stage1, scores): scores
    is a pair of lists of (psnr_y, ssim_y), one for the predictions and - with return_stage1, else empty - one for the stage-1 images, by the
    definitions of tools/evaluate_pairs.py. A batch without ground truth yields the pair. A ground truth of another size raises ValueError before
    anything is launched for its batch. With png the raw result is still not downloaded.
    lpips (with gt only): as in process() - the scored batches yield (psnr_y, ssim_y, lpips) triples.
    niqe (with or without gt): the pristine parameters, as in process(). niqe_rects: an iterable in step with `batches`, advanced like png: per
    batch None - the batch is not scored - or one final size (h, w) per image; without it every batch is scored (with gt: every batch that has
    ground truth) at its png rectangle / resize target / ground truth's size / whole output. ir_niqe_stats is queued behind the paired scores on
    the compute stream, the statistics come back with the batch's download, and the fits and the score run when the batch is yielded. A scored
    batch yields the triple; alone its tuples are (niqe,), with gt the value is appended.
    ilniqe (with or without gt and the other scores): the template, as in process() - ir_ilniqe_stats is queued behind ir_niqe_stats on the batches
    NIQE scores or would score (niqe_rects serves it too), and its value stands right behind NIQE's.
    clipiqa (with or without gt and niqe): as in process() - ir_clipiqa is queued behind ir_niqe_stats on the batches NIQE scores or would score
    (niqe_rects serves both), and its value comes last in every tuple.
    musiq (alone or with gt, lpips, niqe and clipiqa): as in process() - ir_musiq is queued behind ir_clipiqa on the same batches and rectangles, and
    its value comes behind clipiqa's.
    maniqa (alone or with the others): as in process() - ir_maniqa is queued behind ir_musiq on the same batches and rectangles, and its value comes
    last. True, or an iterable in step with the batches that gives each batch's list of names.
    topiq (alone or with the others): as in process() - ir_topiq is queued behind ir_maniqa on the same batches and rectangles, and its value
    comes behind maniqa's and before dists's.
    dists (with gt only): as in process() - the scored batches' tuples end with the DISTS value.
    fid: as in process() - a batch that enters the set yields the features dict as its last element. fid_rects: an iterable in step with the
    batches: per batch one (h, w) per image, or None for a batch that does not enter the set (its saved image is not the device's image);
    without it every batch enters, a batch with gt= only when it has ground truth."""
    noise_scheduler = noise_scheduler or DDPMScheduler()
    if lpips and gt is None:
        raise ValueError("process_stream(lpips=True) needs gt=: LPIPS is scored against the ground truth")
    if dists and gt is None:
        raise ValueError("process_stream(dists=True) needs gt=: DISTS is scored against the ground truth")
    if not _fused_ok(model, preprocess_model, vae, disable_preprocess_model):
        raise TypeError("process_stream needs instarevive_amd models sharing one context")
    ctx, device = model.ctx, model.device
    acp, sf = float(noise_scheduler.alphas_cumprod[400]), float(vae.config.scaling_factor)
    if fp8 and not vae.__dict__.get("_fp8_uploaded"):
        raise RuntimeError("process_stream(fp8=True): call vae.enable_fp8() first - without the fp8 weight forms every layer would silently run in bf16")
    base_flags = _pipeline_flags(model, color_fix_type, disable_preprocess_model, tiled) | (L.FLAG_GRAPH if graph else 0) | (L.FLAG_FP8 if fp8 else 0)
    main, copy = torch.cuda.current_stream(device), ctx.__dict__.setdefault("_copy_stream", torch.cuda.Stream(device))
    it = iter(batches)
    codec = _jpeg_codec(png, jpeg, jpeg_quality, jpeg_subsampling)
    png_it = iter(png) if png is not None else (iter(jpeg) if jpeg is not None else None)
    resize_it = iter(resize) if resize is not None else None
    degrade_it = iter(degrade) if degrade is not None else None
    if degrade_it is not None and resize_it is None:
        raise ValueError("process_stream(degrade=...) needs resize=: the ground truth is degraded on the device input route")
    gt_it = iter(gt) if gt is not None else None
    noref = niqe is not None or ilniqe is not None or bool(clipiqa) or bool(musiq) or bool(maniqa) or bool(topiq)
    mq_it = iter(maniqa) if maniqa and maniqa is not True else None
    nq_it = iter(niqe_rects) if noref and niqe_rects is not None else None
    fid = ("clean" if fid is True else fid) or None
    fid_it = iter(fid_rects) if fid and fid_rects is not None else None

    def staged(batch, slot):
        """The next batch, planned and with its uploads queued on the copy stream. Every per-batch iterable is advanced right after the batch
        has been drawn."""
        rects = next(png_it) if png_it is not None else None
        records = next(resize_it) if resize_it is not None else None
        dparams = next(degrade_it) if degrade_it is not None else None
        if dparams is not None and records is None:
            raise ValueError("process_stream: a batch with degrade records needs resize records")
        gts = next(gt_it) if gt_it is not None else None
        sizes = next(nq_it) if nq_it is not None else None
        with_nq = noref and (sizes is not None if nq_it is not None else (gts is not None or gt_it is None))
        names = next(mq_it) if mq_it is not None else None
        fsizes = next(fid_it) if fid_it is not None else None
        with_fid = fid and (fsizes is not None if fid_it is not None else (gts is not None or gt_it is None))
        imgs, by, bm = _split_batch(batch)
        b = _Batch(ctx, slot, "stream", 2, _batch_shape(imgs, records), imgs, return_stage1, rects, records, dparams, gts, lpips,
                   niqe if with_nq else None, bool(clipiqa) and with_nq, sizes, lq_sink is not None, (by, bm), codec=codec, png_runs=png_runs, musiq=bool(musiq) and with_nq,
                   maniqa=(names if names is not None else True) if maniqa and with_nq else False, dists=dists,
                   fid=fid if with_fid else None, fid_sizes=fsizes, ilniqe=ilniqe if with_nq else None, topiq=bool(topiq) and with_nq)
        with torch.cuda.stream(copy):
            b.ready = b.upload(copy, main)
        return b

    def finished(b):
        b.done.synchronize()
        if b.want_lq:
            lq_sink(b.host_lq())
        return b.collect(copy, png_wrap)

    last_prompt = None   # the host prompts of the last triple batch that were set (a batch with the same ones sets nothing)

    def set_batch_prompt(by, bm, n):
        nonlocal last_prompt
        if by is None:
            if last_prompt is not None:   # back to the run's own prompt after per-batch ones
                model.invalidate_prompt()
                last_prompt = None
            model.set_prompt(y, y_mask)
            return
        key = getattr(by, "text_prompt_key", None)
        if key is not None:   # a batch that text_prompts.PromptSource.batch() marked: its prompts stay on the device. The key names their contents, so
            # the two things the host route does by comparing tensors are done on the key: equal prompts as one slot, an unchanged batch sets nothing
            if len(key) not in (1, n):
                raise ValueError(f"process_stream: a batch of {n} images came with {len(key)} prompts (one, or one per image)")
            if last_prompt is not None and last_prompt[0] is None and last_prompt[1] == key:
                return
            rows = 1 if len(set(key)) == 1 else len(key)
            yd = by.detach().reshape(len(key), by.shape[-2], by.shape[-1])[:rows].contiguous()
            model.set_prompts_device(yd, bm.detach().reshape(len(key), by.shape[-2])[:rows].contiguous())
            last_prompt = (None, key)
            return
        hy = by.detach().to("cpu", torch.float32)
        hy = hy.reshape(-1, hy.shape[-2], hy.shape[-1])
        hb = prompt_bias(bm, hy.shape[0], hy.shape[1])
        if hy.shape[0] not in (1, n):
            raise ValueError(f"process_stream: a batch of {n} images came with {hy.shape[0]} prompts (one, or one per image)")
        if last_prompt is not None and last_prompt[0] is not None and torch.equal(last_prompt[0], hy) and torch.equal(last_prompt[1], hb):
            return
        model._set_prompt_rows(hy, hb, stream_ordered=True)
        last_prompt = (hy, hb)

    pending = None
    nxt = next(it, None)
    cur = staged(nxt, 0) if nxt is not None else None
    while cur is not None:
        n, h, w = cur.shape
        _prepare_fused(model, y, y_mask, h, w, tiled, tile_size, (vae, None if disable_preprocess_model else preprocess_model), set_prompt=False)
        set_batch_prompt(*cur.prompts, n)
        main.wait_event(cur.ready)
        cur.reserve()
        cur.launch(base_flags, tile_size, tile_stride, acp, sf)
        computed = torch.cuda.Event()
        computed.record(main)
        # while this batch computes: fetch the previous result, stage the next input into the other slot. The other slot's device
        # buffers were last read by the previous batch's download, which finished() has waited for by then.
        if pending is not None:
            yield finished(pending)
        nxt = next(it, None)
        up = staged(nxt, cur.slot ^ 1) if nxt is not None else None
        with torch.cuda.stream(copy):
            copy.wait_event(computed)
            cur.download()
            cur.done = torch.cuda.Event()
            cur.done.record(copy)
        pending, cur = cur, up
    if pending is not None:
        yield finished(pending)


class HipTileEngine:
    """The five phases of tiled sampling (ir_tiled_* of the C ABI) on one GPU, in the form parallel.sharded_tiled_process() drives:
    every rank encodes, each rank runs the DiT / the decoder on ITS tiles, the per-tile results are exchanged between the phases."""

    def __init__(self, model, vae, preprocess_model, y, y_mask, color_fix_type="wavelet", disable_preprocess_model=False, tile_size=512,
                 tile_stride=448, noise_scheduler=None):
        if not _fused_ok(model, preprocess_model, vae, disable_preprocess_model):
            raise TypeError("HipTileEngine needs instarevive_amd models sharing one context")
        self.model, self.ctx, self.device = model, model.ctx, model.device
        self.others = (vae, None if disable_preprocess_model else preprocess_model)
        self.y, self.y_mask = y, y_mask
        self.tile_size, self.tile_stride = tile_size, tile_stride
        self.flags = _pipeline_flags(model, color_fix_type, disable_preprocess_model, True)
        sch = noise_scheduler or DDPMScheduler()
        self.acp, self.sf = float(sch.alphas_cumprod[400]), float(vae.config.scaling_factor)

    def _ws(self):
        n, h, w = self.shape
        return self.ctx.workspace(self.ctx.ws_bytes(L.STAGE_PIPELINE, n, h, w, self.flags, self.tile_size, self.tile_stride))

    def count(self, h, w):
        k = self.ctx.lib.ir_tiled_count(h, w, self.tile_size, self.tile_stride)
        if k <= 0:
            raise ValueError(f"bad tile geometry for a {h}x{w} image: tile {self.tile_size}, stride {self.tile_stride}")
        return k

    def encode(self, control_imgs):
        n, h, w = _check_images(control_imgs)
        self.shape = (n, h, w)
        _prepare_fused(self.model, self.y, self.y_mask, h, w, True, self.tile_size, self.others)
        st = _Staging.get(self.ctx, n, h, w)
        st.fill(0, control_imgs)
        st.upload(0)
        control = torch.empty((n, 3, h, w), dtype=torch.float32, device=self.device)
        init = torch.empty((n, 4, h // 8, w // 8), dtype=torch.float32, device=self.device)
        ws = self._ws()
        c = self.ctx
        c.check(c.lib.ir_tiled_encode(c.h, c.stream(), L.ptr(st.d_in[0]), L.ptr(st.d_st1[0]), L.ptr(control), L.ptr(init), n, h, w, self.flags,
                                      self.sf, L.ptr(ws), ws.numel()), "ir_tiled_encode")
        self._stage1 = st.d_st1[0]
        return control, init

    def can_shard_encode(self, control_imgs):
        """The encoder's mid-block attention can be split by query rows: one image, 512-channel mid block, h * w / 64 a multiple of 128."""
        n, h, w = _check_images(control_imgs)
        vae = self.others[0]
        return n == 1 and ((h // 8) * (w // 8)) % 128 == 0 and vae.config.block_out_channels[-1] == 512

    def encode_overflow(self):
        """1 when the fixed softmax reference of the last encode_part0 overflowed on THIS rank's rows (all rows of attn_o were then
        recomputed by the rescaling kernel), else 0. Synchronises the stream."""
        c = self.ctx
        v = c.lib.ir_tiled_encode_overflow(c.h, c.stream())
        if v < 0:
            c.check(v, "ir_tiled_encode_overflow")
        return int(v)

    def encode_part0(self, control_imgs, row0, row1, force_fallback=False):
        """ir_tiled_encode_part(part 0): everything up to the attention of query rows [row0, row1) of the encoder's mid block. Returns
        (control, attn_o, attn_res): this rank's rows of attn_o are filled; the exchange of the rows is the caller's (parallel.py)."""
        n, h, w = _check_images(control_imgs)
        self.shape = (n, h, w)
        _prepare_fused(self.model, self.y, self.y_mask, h, w, True, self.tile_size, self.others)
        st = _Staging.get(self.ctx, n, h, w)
        st.fill(0, control_imgs)
        st.upload(0)
        T = (h // 8) * (w // 8)
        control = torch.empty((n, 3, h, w), dtype=torch.float32, device=self.device)
        self._init = torch.empty((n, 4, h // 8, w // 8), dtype=torch.float32, device=self.device)
        attn_o = torch.empty((T, 512), dtype=torch.bfloat16, device=self.device)
        attn_res = torch.empty((T, 512), dtype=torch.bfloat16, device=self.device)
        ws, c = self._ws(), self.ctx
        c.check(c.lib.ir_tiled_encode_part(c.h, c.stream(), L.ptr(st.d_in[0]), L.ptr(st.d_st1[0]), L.ptr(control), L.ptr(self._init), n, h, w, self.flags,
                                           self.sf, 2 if force_fallback else 0, row0, row1, L.ptr(attn_o), L.ptr(attn_res), L.ptr(ws), ws.numel()),
                "ir_tiled_encode_part(0)")
        self._stage1 = st.d_st1[0]
        return control, attn_o, attn_res

    def encode_part1(self, control, attn_o, attn_res):
        """ir_tiled_encode_part(part 1): the rest of the encoder from all rows of attn_o. Returns init."""
        n, h, w = self.shape
        ws, c = self._ws(), self.ctx
        c.check(c.lib.ir_tiled_encode_part(c.h, c.stream(), None, None, L.ptr(control), L.ptr(self._init), n, h, w, self.flags, self.sf, 1, 0, 0,
                                           L.ptr(attn_o), L.ptr(attn_res), L.ptr(ws), ws.numel()), "ir_tiled_encode_part(1)")
        return self._init

    def stage1(self):
        n = self.shape[0]
        a = self._stage1.cpu().numpy()
        return [a[i] for i in range(n)]

    def dit_tiles(self, init, first, step):
        n, h, w = self.shape
        k = len(range(first, self.count(h, w), step))
        tl = self.tile_size // 8
        x0 = torch.empty((max(k, 1), n, 4, tl, tl), dtype=torch.float32, device=self.device)
        ws, c = self._ws(), self.ctx
        c.check(c.lib.ir_tiled_dit(c.h, c.stream(), L.ptr(init), L.ptr(x0), n, h, w, self.tile_size, self.tile_stride, first, step, 400.0, self.acp,
                                   self.flags, L.ptr(ws), ws.numel()), "ir_tiled_dit")
        return x0[:k]

    def blend_latent(self, x0_all):
        n, h, w = self.shape
        nb = torch.empty((n, 4, h // 8, w // 8), dtype=torch.float32, device=self.device)
        c = self.ctx
        c.check(c.lib.ir_tiled_blend_latent(c.h, c.stream(), L.ptr(x0_all.contiguous()), L.ptr(nb), n, h, w, self.tile_size, self.tile_stride),
                "ir_tiled_blend_latent")
        return nb

    def decode_tiles(self, nb, control, first, step):
        n, h, w = self.shape
        k = len(range(first, self.count(h, w), step))
        tp = (self.tile_size // 8) * 8
        px = torch.empty((max(k, 1), n, 3, tp, tp), dtype=torch.float32, device=self.device)
        ws, c = self._ws(), self.ctx
        c.check(c.lib.ir_tiled_decode(c.h, c.stream(), L.ptr(nb), L.ptr(control), L.ptr(px), n, h, w, self.tile_size, self.tile_stride, first, step,
                                      self.flags, self.sf, L.ptr(ws), ws.numel()), "ir_tiled_decode")
        return px[:k]

    def blend_pixels(self, px_all, png=None, png_runs=False):
        """The assembled uint8 frames; with png (one valid rectangle per image) their PNG files, encoded on this GPU (png_runs: in the run mode), as bytes."""
        n, h, w = self.shape
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=self.device)
        ws, c = self._ws(), self.ctx
        c.check(c.lib.ir_tiled_blend_pixels(c.h, c.stream(), L.ptr(px_all.contiguous()), L.ptr(out), n, h, w, self.tile_size, self.tile_stride,
                                            L.ptr(ws), ws.numel()), "ir_tiled_blend_pixels")
        if png is not None:
            enc = _png_encoder(c, n, h, w, 0, "tiles", png_runs)
            enc.queue(0, out, png)
            enc.fetch_sizes()
            torch.cuda.current_stream(self.device).synchronize()
            return enc.fetch(n)
        a = out.cpu().numpy()
        return [a[i] for i in range(n)]
