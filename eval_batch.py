#!/usr/bin/env python3
"""Batched evaluation harness of the one-step path — the role of the reference's test_scripts/test_dmd_general.py:112-192 (and
test_dmd.py:111-185 for the face weights): a folder of low-quality images goes through the network in batches of B and two folders come
out, the restored images and the stage-1 ("condition") images, each under its input's file name (`.jpg` -> `.png`, like save_batch,
test_dmd_general.py:37-51).

    python eval_batch.py --ckpt weights/InstaRevive_v1.ckpt --input DIR --output OUT_DIR --cond_output COND_DIR [--batch_size 4]
                         [--image_size 512] [--swinir_ckpt weights/face_swinir_v1.ckpt] [--prompt_embeds face_prompt.pth] ...

What the reference's harness builds with its dataset classes (synthetic degradation of ground-truth images, which SURVEY.md section 2.2
puts out of scope) is replaced by the file list of an EXISTING low-quality folder; every image is centre-cropped to image_size
(center_crop_arr, utils/image/common.py:12-36 — the reference's face / general evaluation feeds 512 x 512 crops), so a batch is
uniform and B images share every kernel launch. The per-batch arithmetic is the reference loop's: SwinIR -> VAE encode (mode) x scaling
factor -> generate_sample_1step at t = 400 -> VAE decode / 2 + 0.5 (:156-186), i.e. process() without tiling.
Model / prompt / scheduler artefacts are the ones of inference.py; the face variant differs only in --swinir_ckpt and --prompt_embeds.
With torchrun the file list is sharded over the ranks.
"""
import os
from argparse import ArgumentParser
from collections import deque

import numpy as np
import torch
from PIL import Image

import inference as cli


def parse_args():
    ap = ArgumentParser()
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--cond_output", default=None, help="folder for the stage-1 (condition) images; default: <output>-cond")
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--disable_preprocess_model", action="store_true")
    ap.add_argument("--swinir_ckpt", default="./weights/general_swinir_v1.ckpt")
    ap.add_argument("--swinir_config", default="./configs/swinir.yaml")
    ap.add_argument("--vae", default="stabilityai/sd-vae-ft-ema")
    ap.add_argument("--dit_config", default="PixArt-alpha/PixArt-Alpha-DMD-XL-2-512x512")
    ap.add_argument("--prompt_embeds", default=cli.DEFAULT_PROMPT)
    ap.add_argument("--caption_dir", default=None, help="per-image prompts: DIR/<input-relative path without extension>.npz, else DIR/<file stem>.npz "
                    "(caption_feature [1, T, 4096], optional attention_mask; the reference's caption files). Images without one get --prompt_embeds")
    cli.add_text_prompt_flags(ap)   # --prompt, --captions, --t5 / --t5_pipeline, --prompt_max_length, --clean_captions, --save_captions: as in inference.py
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--png_encoder", default="host", choices=["host", "gpu"], help="who compresses the PNGs of both output folders: the host (PIL, default) or "
                    "the GPU behind the network (inference.py --png_encoder: lossless, meant for photographs; flat content comes out larger than PIL's unless "
                    "--png_runs is given)")
    ap.add_argument("--png_runs", action="store_true", help="with --png_encoder gpu: the device encoder's run mode (inference.py --png_runs: runs of equal "
                    "filtered bytes coded as matches, the same pixels, no file larger, flat content several times smaller)")
    cli.add_jpeg_flags(ap)   # --save_format jpg, --jpeg_quality, --jpeg_subsampling, --jpeg_encoder: as in inference.py, for both output folders
    ap.add_argument("--gt", default=None, help="score both output folders against ground truth on the GPU (inference.py --gt: PSNR-Y / SSIM-Y, the same lookup "
                    "rules); the ground truth is centre-cropped to --image_size like the input. Writes metrics.csv (metrics.rank<k>.csv with several ranks) into "
                    "--output and --cond_output and prints both averages")
    ap.add_argument("--lpips_lin", default=None, help="with --gt: LPIPS (v0.1, alex) on the GPU as a fourth CSV column and a `lpips:` average line "
                    "(inference.py --lpips_lin: the lpips linear heads, or a full lpips.LPIPS() state dict); --image_size must be at least 31")
    ap.add_argument("--lpips_alexnet", default=None, help="with --lpips_lin holding the heads alone: torchvision's AlexNet state dict")
    ap.add_argument("--dists_model", default=None, metavar="FILE", help="with --gt (or --degrade): DISTS on the GPU as the last CSV column and a `dists:` average line "
                    "(inference.py --dists_model: a DISTS state dict, alpha / beta with --dists_vgg, or an .npz); --image_size must be at least 16")
    ap.add_argument("--dists_vgg", default=None, metavar="FILE", help="with --dists_model holding alpha / beta alone: torchvision's VGG-16 state dict")
    ap.add_argument("--fid_model", default=None, metavar="FILE", help="FID of the restored folder on the GPU (inference.py --fid_model: pytorch-fid's pt_inception state "
                    "dict or an .npz) against the ground truth of the scored files (--gt or --degrade) or against --fid_stats; with neither it is refused. One last "
                    "line `fid: x.xxxxx` behind the averages; the CSVs do not change")
    ap.add_argument("--fid_resize", default="clean", choices=["clean", "legacy"], help="with --fid_model: clean (pyiqa / clean-fid: Pillow's float BICUBIC) or legacy (pytorch-fid: torch's bilinear)")
    ap.add_argument("--fid_stats", default=None, metavar="FILE.npz", help="with --fid_model: the reference set's statistics (pytorch-fid's mu / sigma); needs no --gt")
    ap.add_argument("--fid_features_out", default=None, metavar="FILE", help="with --fid_model: where the run's features go (default <output>/fid_features.npz; fid_features.rank<k>.npz with several ranks)")
    ap.add_argument("--niqe_params", default=None, help="score NIQE (no reference needed) of both output folders on the GPU (inference.py --niqe_params: "
                    "niqe_modelparameters.mat or an .npz). Works without --gt: the CSVs are then file,niqe; with --gt the column comes last. --image_size must "
                    "be at least 192 for two blocks")
    ap.add_argument("--ilniqe_params", default=None, help="score IL-NIQE (no reference needed) of both output folders on the GPU (inference.py --ilniqe_params: "
                    "ILNIQE_templateModel.mat or an .npz). Works with or without --gt and the other metric flags; its column stands right behind niqe's place")
    ap.add_argument("--clipiqa_model", default=None, help="score CLIP-IQA (no reference needed) of both output folders on the GPU (inference.py --clipiqa_model: "
                    "OpenAI's RN50.pt or an .npz). Works with or without --gt and --niqe_params; its column comes last. --image_size must be at least 32")
    ap.add_argument("--musiq_model", default=None, help="score MUSIQ (no reference needed) of both output folders on the GPU (inference.py --musiq_model: an .npz "
                    "in tools/evaluate_musiq.py's names or pyiqa's .pth). Works with or without --gt, --niqe_params and --clipiqa_model; its column comes last")
    ap.add_argument("--maniqa_model", default=None, help="score MANIQA (no reference needed) of both output folders on the GPU (inference.py --maniqa_model: an .npz "
                    "in tools/evaluate_maniqa.py's names or pyiqa's .pth). Works with or without --gt and the other scorers; its column comes last. --image_size "
                    "must be above 224")
    ap.add_argument("--topiq_model", default=None, help="score TOPIQ-NR (no reference needed) of both output folders on the GPU (inference.py --topiq_model: an .npz "
                    "in tools/evaluate_topiq.py's names or pyiqa's .pth). Works with or without --gt and the other scorers; its column comes behind maniqa's "
                    "and before dists's. --image_size below 16 leaves every file unscored")
    ap.add_argument("--maniqa_crops", default="uniform", choices=["uniform", "random"], help="inference.py's flag: pyiqa's grid, or draws from --maniqa_seed and the saved file's name")
    ap.add_argument("--maniqa_seed", type=int, default=None, help="with --maniqa_crops random: the seed (default 231)")
    ap.add_argument("--clip_bpe", default=None, help="with --clipiqa_model: the folder that holds CLIP's BPE table (inference.py --clip_bpe)")
    ap.add_argument("--degrade", nargs="?", const="lq", default=None, metavar="lq|realesrgan|FILE.json", help="--input holds GROUND TRUTH: the centre crops are degraded on "
                    "the GPU (inference.py --degrade: blur, bilinear downsample, noise, JPEG, bilinear resize back; `realesrgan`: the reference's second-order "
                    "validation recipe) and the LQ images restored (with --center_crop gpu the crops are made on the device as well); needs "
                    "--image_size to be a multiple of 64 of at least 512 (the crop is then the network input as it is). Without --gt the input folder "
                    "is the ground truth of --lpips_lin / --niqe_params / --clipiqa_model / --musiq_model / --maniqa_model")
    ap.add_argument("--degrade_seed", type=int, default=231, help="with --degrade: seeds every file's draws together with the crc32 of its input-relative path")
    ap.add_argument("--save_lq", default=None, metavar="DIR", help="with --degrade: write the synthesised LQ crops to DIR")
    ap.add_argument("--jpeg_decoder", default="host", choices=["host", "gpu"], help="inference.py's flag; `gpu` only together with --center_crop gpu: without it "
                    "every input is centre-cropped on the host (a BOX filter halves large files), which inference.py --jpeg_decoder gpu refuses as --use_center_crop")
    ap.add_argument("--png_decoder", default="host", choices=["host", "gpu"], help="inference.py's flag, under --jpeg_decoder's condition: `gpu` only together "
                    "with --center_crop gpu. Both decoder flags may be given")
    ap.add_argument("--center_crop", default="host", choices=["host", "gpu"], help="who centre-crops the inputs to --image_size. host (default): PIL on the reader "
                    "threads (center_crop_arr). gpu: the decoded file - with --jpeg_decoder gpu the compressed bytes of a baseline JPEG - is uploaded and the "
                    "device makes the same pixels (inference.py --center_crop gpu: BOX halvings, the bicubic resize, the central window); with --degrade the crop "
                    "is then degraded on the device as well. The ground-truth files of --gt stay decoded and cropped on the host")
    ap.add_argument("--workers", type=int, default=-1, help="host threads for decoding / PNG encoding (inference.py --workers)")
    return ap.parse_args()


def out_name(folder, src_root, path, ext_out=".png"):
    rel = os.path.relpath(path, src_root)
    stem, ext = os.path.splitext(rel)
    if ext_out == ".jpg":   # --save_format jpg: every file is a JPEG
        return os.path.join(folder, stem + ".jpg")
    return os.path.join(folder, stem + ".png" if ext.lower() in (".jpg", ".jpeg") else rel)


def main():
    from instarevive_amd import parallel
    from instarevive_amd.pipeline import process_stream
    from instarevive_amd.prompts import Captions
    from instarevive_amd.resample import ResizeJob, crop_geometry
    from instarevive_amd.utils import center_crop_arr, list_image_files
    args = parse_args()
    cli.check_text_prompts(args)
    cli.check_save_format(args)
    crop_gpu = args.center_crop == "gpu"
    if args.jpeg_decoder == "gpu" and crop_gpu:
        args.jpeg_decode_log = []   # per file None (decoded on the device) or the reason it took the host decoder
    elif args.jpeg_decoder == "gpu":
        raise SystemExit("--jpeg_decoder gpu decodes into the device's resize route, and this tool centre-crops every input on the host (as inference.py "
                         "--use_center_crop, where the flag is refused too): not offered (or give --center_crop gpu)")
    if args.png_decoder == "gpu" and crop_gpu:
        args.png_decode_log = []
    elif args.png_decoder == "gpu":
        raise SystemExit("--png_decoder gpu decodes into the device's resize route, and this tool centre-crops every input on the host (as inference.py "
                         "--use_center_crop, where the flag is refused too): not offered (or give --center_crop gpu)")
    ext_out = cli.save_ext(args)
    topiq_model = cli.load_topiq_model(args)
    niqe_params = cli.load_niqe_params(args)
    ilniqe_params = cli.load_ilniqe_params(args)
    clipiqa_model = cli.load_clipiqa_model(args)
    musiq_model = cli.load_musiq_model(args)
    maniqa_model = cli.load_maniqa_model(args)
    dists_weights = cli.load_dists_weights(args)
    fid_weights, fid_stats = cli.load_fid(args)
    noref = bool(niqe_params) or ilniqe_params is not None or clipiqa_model is not None or musiq_model is not None or maniqa_model is not None or topiq_model is not None
    recipe = geo = None
    if args.save_lq and not args.degrade:
        raise SystemExit("--save_lq writes the images --degrade synthesises: give --degrade as well")
    if args.degrade:
        from instarevive_amd import degrade as D
        from instarevive_amd.resample import job_geometry
        try:
            recipe = D.load_recipe(args.degrade)
        except (D.DegradeError, OSError, ValueError) as e:
            raise SystemExit(f"--degrade: {e}")
        geo = job_geometry((args.image_size, args.image_size), 1, False, 512)   # the device input route of inference.py --resize gpu
        if geo.chain or geo.net_hw != (args.image_size, args.image_size):
            raise SystemExit("--degrade needs --image_size to be a multiple of 64 of at least 512 (the crop is the network input as it is)")
        if not args.gt and (args.lpips_lin or noref or dists_weights or (fid_weights and fid_stats is None)):
            args.gt = args.input   # the files that are degraded are the ground truth of what is restored from them
    cli.check_device(args.device)
    rank, world, local = parallel.init_distributed()
    torch.cuda.set_device(local)
    m = cli.load_models(args, torch.device("cuda", local))
    from instarevive_amd import text_prompts
    text_caps = text_prompts.setup(args, m, torch.device("cuda", local), log=lambda t: print(f"[rank {rank}] {t}"), max_batch=max(args.batch_size, 1))
    cond_dir = args.cond_output or args.output.rstrip("/") + "-cond"
    fid_run = None
    if fid_weights:
        from instarevive_amd import fid
        fid.configure(m.model.ctx, fid_weights)
        fid_run = fid.Run(fid.Run.default_path(args.output, args.fid_features_out), fid_stats, rank, world)
    # os.walk order is filesystem-dependent: every rank sorts its listing and takes rank 0's copy, so that ownership of a file follows from
    # ONE list (the same rule as inference.py)
    files = sorted(list_image_files(args.input, follow_links=True))
    if world > 1:
        files = parallel.agree_on_list(files)
    files = parallel.shard(files, rank, world)
    batches = [files[i:i + args.batch_size] for i in range(0, len(files), args.batch_size)]
    pools = cli.HostPools(cli.default_workers(int(os.environ.get("LOCAL_WORLD_SIZE", world))) if args.workers < 0 else args.workers)

    caps = Captions(args.caption_dir, m.y, m.y_mask, args.input) if args.caption_dir else text_caps   # --captions: the same per-batch path, prompts on the device

    reports, truths, records, dparams, lq_images = None, deque(), deque(), deque(), []
    if (args.lpips_lin or args.lpips_alexnet) and not args.gt:
        raise SystemExit("--lpips_lin / --lpips_alexnet score against ground truth: give --gt as well")
    if args.lpips_alexnet and not args.lpips_lin:
        raise SystemExit("--lpips_alexnet needs --lpips_lin (the lpips linear heads)")
    with_lpips = {"lpips": True} if args.lpips_lin else {}
    with_niqe = {**({"niqe": True} if niqe_params else {}), **({"ilniqe": True} if ilniqe_params else {}), **({"clipiqa": True} if clipiqa_model else {}), **({"musiq": True} if musiq_model else {}),
                 **({"maniqa": True} if maniqa_model else {}), **({"paired": bool(args.gt)} if noref else {}), **({"dists": True} if dists_weights else {}), **({"topiq_nr": True} if topiq_model else {})}
    lookup = None
    if args.gt or noref:
        from instarevive_amd.metrics import GroundTruth, Report
        lookup = GroundTruth(args.gt, args.input) if args.gt else None
        name = "metrics.csv" if world == 1 else f"metrics.rank{rank}.csv"
        reports = (Report(os.path.join(args.output, name), **with_lpips, **with_niqe), Report(os.path.join(cond_dir, name), **with_lpips, **with_niqe))
        if args.lpips_lin:
            from instarevive_amd import lpips
            lpips.configure(m.model.ctx, args.lpips_lin, args.lpips_alexnet)
        if dists_weights:
            from instarevive_amd import dists
            dists.configure(m.model.ctx, dists_weights)
        if ilniqe_params:
            from instarevive_amd import ilniqe
            ilniqe.configure(m.model.ctx)
        if clipiqa_model:
            from instarevive_amd import clipiqa
            clipiqa.configure(m.model.ctx, clipiqa_model)
        if musiq_model:
            from instarevive_amd import musiq
            musiq.configure(m.model.ctx, musiq_model)
        if maniqa_model:
            from instarevive_amd import maniqa
            maniqa.configure(m.model.ctx, maniqa_model, args.maniqa_crops, args.maniqa_seed)
        if topiq_model:
            from instarevive_amd import topiq
            topiq.configure(m.model.ctx, topiq_model)

    def read(f):
        gt = np.ascontiguousarray(center_crop_arr(lookup.load(f), args.image_size)) if lookup else None
        if crop_gpu:   # decode only (--jpeg_decoder gpu: the headers and one byte pass); the device crops, and degrades the crop
            source = cli.device_source(f, args)   # --jpeg_decoder gpu / --png_decoder gpu
            raw = np.array(Image.open(f).convert("RGB")) if source is None else source
            job = ResizeJob(raw, crop_geometry((raw.shape[1], raw.shape[0]), 1, args.image_size))
            if recipe is None:
                return job, gt
            return job, gt, D.draw(recipe, os.path.relpath(f, args.input), args.image_size, args.image_size, args.degrade_seed)
        crop = center_crop_arr(Image.open(f).convert("RGB"), args.image_size)
        if recipe is None:
            return crop, gt
        crop = np.ascontiguousarray(crop)   # the draws (and the noise field) are made here, on a reader thread
        return crop, gt, D.draw(recipe, os.path.relpath(f, args.input), crop.shape[0], crop.shape[1], args.degrade_seed)

    def feed():
        # decode + centre crop run ahead of the GPU on the reader threads, in file order
        crops = pools.read_ahead(read, files)
        for group in batches:
            pairs = [next(crops) for _ in group]
            imgs = [None if crop_gpu else p[0] for p in pairs]
            truths.append([p[1] for p in pairs])
            if crop_gpu:
                records.append([p[0] for p in pairs])
            elif recipe is not None:
                records.append([ResizeJob(p[0], geo) for p in pairs])
            if recipe is not None:
                dparams.append([p[2] for p in pairs])
            yield (imgs, *caps.batch(group)) if caps else imgs

    def save(dst, img):
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        if isinstance(img, tuple):   # encoded on the GPU: (zlib stream, width, height) or a JPEG's six pieces, framed here on the writer thread
            from instarevive_amd.jpeg import wrap_jpeg
            from instarevive_amd.png import wrap_png
            with open(dst, "wb") as f:
                f.write(wrap_png(*img) if len(img) == 3 else wrap_jpeg(*img))
        elif dst.endswith(".jpg") and ext_out == ".jpg":
            from instarevive_amd.jpeg import save_host, subsampling_of
            save_host(Image.fromarray(np.ascontiguousarray(img)), dst, args.jpeg_quality, subsampling_of(args.jpeg_subsampling))
        else:
            Image.fromarray(np.ascontiguousarray(img)).save(dst)

    gpu_jpg = ext_out == ".jpg" and args.jpeg_encoder == "gpu"
    whole = [[(args.image_size, args.image_size)] * len(group) for group in batches]
    if ext_out == ".jpg" and (args.gt or noref):
        print(f"[rank {rank}] --save_format jpg: the scores are those of the device's image, the result BEFORE the JPEG loss")
    gpu_png = args.png_encoder == "gpu"   # every image is a whole image_size crop: nothing to un-pad, every file is eligible

    results = process_stream(m.model, feed(), "none", args.disable_preprocess_model, False, 512, 448, preprocess_model=m.preprocess_model, vae=m.vae,
                             y=m.y, y_mask=m.y_mask, noise_scheduler=m.noise_scheduler, return_stage1=True,
                             png=whole if gpu_png else None, png_wrap=False, png_runs=args.png_runs,
                             **({"jpeg": whole, "jpeg_quality": args.jpeg_quality, "jpeg_subsampling": args.jpeg_subsampling} if gpu_jpg else {}),
                             gt=cli.in_step(truths) if lookup else None, **with_lpips, **({"niqe": niqe_params} if niqe_params else {}), **({"ilniqe": ilniqe_params} if ilniqe_params else {}),
                             **({"clipiqa": True} if clipiqa_model else {}), **({"musiq": True} if musiq_model else {}), **({"dists": True} if dists_weights else {}),
                             **({"topiq": True} if topiq_model else {}),
                             **({"fid": args.fid_resize} if fid_run else {}),
                             **({"maniqa": [[os.path.basename(out_name(args.output, args.input, f, ext_out)) for f in group] for group in batches]} if maniqa_model else {}),
                             **({"resize": cli.in_step(records)} if recipe or crop_gpu else {}),
                             **({"degrade": cli.in_step(dparams), "lq_sink": lq_images.append if args.save_lq else None} if recipe else {}))
    no_score = {"niqe": 0, "ilniqe": 0, "clipiqa": 0, "musiq": 0, "maniqa": 0, "topiq_nr": 0, "dists": 0}
    for group, out in zip(batches, results):
        preds, stage1 = out[:2]
        if fid_run:   # every image is a whole crop saved as the device leaves it: every file enters the set
            fid_run.add([os.path.relpath(out_name(args.output, args.input, f, ext_out), args.output) for f in group], out[-1])
            out = out[:-1]
        if reports:
            for rep, folder, scores in zip(reports, (args.output, cond_dir), out[2]):
                for f, score in zip(group, scores):
                    missing = rep.unscored(score)   # NaN: the image has no NIQE, no CLIP-IQA, no MUSIQ or no MANIQA
                    if missing:
                        no_score[missing] += 1
                    else:
                        rep.add_scores(os.path.relpath(out_name(folder, args.input, f, ext_out), folder), score)
        for f, pred, cond in zip(group, preds, stage1):
            for folder, img in ((args.output, pred), (cond_dir, cond)):
                pools.write_behind(save, out_name(folder, args.input, f, ext_out), img)
        if args.save_lq:
            for f, lq in zip(group, lq_images.pop(0)):
                pools.write_behind(save, os.path.splitext(os.path.join(args.save_lq, os.path.relpath(f, args.input)))[0] + ".png", lq)
                pools.written -= 1   # a file counts by its results
        print(f"[rank {rank}] queued {len(group)} images ({group[0]} ...)")
    pools.drain()
    if text_caps:
        text_caps.finish()   # the device's status word: nothing outside the vocabulary or the cache reached it
        print(f"[rank {rank}] --captions: {text_caps.encoded} captions were T5-encoded in the run" + (f", {len(text_caps.saved)} caption files written to {args.save_captions}" if args.save_captions else ""))
    print(f"[rank {rank}] saved {pools.written} files")
    if cli.jpeg_decoder_note(args):
        print(f"[rank {rank}] {cli.jpeg_decoder_note(args)}")
    if cli.png_decoder_note(args):
        print(f"[rank {rank}] {cli.png_decoder_note(args)}")
    if gpu_png:
        print(f"[rank {rank}] --png_encoder gpu: 0 of {pools.written} files took the host encoder")
    if gpu_jpg:
        print(f"[rank {rank}] --jpeg_encoder gpu: {pools.written} of {pools.written} files were coded on the device, 0 took the host encoder")
    if reports:
        for rep, folder in zip(reports, (args.output, cond_dir)):
            lines = rep.write()
            print(f"[rank {rank}] {' / '.join(f for f, on in (('--gt', args.gt), ('--niqe_params', niqe_params), ('--ilniqe_params', ilniqe_params), ('--clipiqa_model', clipiqa_model), ('--musiq_model', musiq_model), ('--maniqa_model', maniqa_model), ('--topiq_model', topiq_model)) if on)}: scored {len(rep.rows)} files of {folder}"
                  + (f" against {args.gt}" if args.gt else "") + f" -> {rep.path}")
            for ln in lines:
                print(ln)
        if no_score["clipiqa"]:
            print(f"[rank {rank}] --clipiqa_model: {no_score['clipiqa']} files were not scored (CLIP-IQA needs 32 x 32 pixels)")
        if no_score["musiq"]:
            print(f"[rank {rank}] --musiq_model: {no_score['musiq']} files were not scored (a resized side rounds to 0)")
        if no_score["maniqa"]:
            print(f"[rank {rank}] --maniqa_model: {no_score['maniqa']} files were not scored (MANIQA needs a short side above 224 pixels)")
        if no_score["topiq_nr"]:
            print(f"[rank {rank}] --topiq_model: {no_score['topiq_nr']} files were not scored (TOPIQ-NR needs 16 x 16 pixels)")
        if no_score["niqe"]:
            print(f"[rank {rank}] --niqe_params: {no_score['niqe']} files were not scored (NIQE needs 96 x 96 blocks and two complete feature rows)")
        if no_score["ilniqe"]:
            print(f"[rank {rank}] --ilniqe_params: {no_score['ilniqe']} files were not scored (IL-NIQE needs two complete feature rows)")
        if no_score["dists"]:
            print(f"[rank {rank}] --dists_model: {no_score['dists']} files were not scored (DISTS is scored from 16 x 16 pixels)")
    if fid_run:
        fid_run.finish()


if __name__ == "__main__":
    main()
