#!/usr/bin/env python3
"""Drop-in for the reference's SR command line (test_scripts/inference.py, documented in README.md:57,63):

    python inference.py --ckpt weights/InstaRevive_v1.ckpt --input DIR --output DIR [--sr_scale F] [--tiled
        --tile_size 512 --tile_stride 448] [--color_fix_type wavelet|adain|none] [--disable_preprocess_model] ...

Same flags, defaults, file naming (`<stem>_<i>.png` under the input's relative path; `.jpg` with --save_format jpg) and artefacts:
  * DiT:      flat state dict in diffusers Transformer2DModel key layout  (--ckpt; the reference parses --ckpt but
              hard-codes ./weights/InstaRevive_v1.ckpt, inference.py:239-240 — here --ckpt is honoured)
  * SwinIR:   ./weights/general_swinir_v1.ckpt with ./configs/swinir.yaml     (override: --swinir_ckpt / --swinir_config)
  * VAE:      diffusers folder 'stabilityai/sd-vae-ft-ema'                     (override: --vae)
  * prompt:   {'caption_embeds': [1,300,4096], 'emb_mask': [1,300]} .pth       (override: --prompt_embeds)
  * scheduler: only alphas_cumprod[400] is consumed                            (override: --dit_config folder)
All compute runs on the MI355X through hand-written HIP kernels; `--device cpu|mps` is rejected (no CPU path).
With torchrun (WORLD_SIZE > 1) the file list is sharded over the ranks, one process per GPU (images are independent); with
--tiled --shard_tiles the tiles of each image are sharded instead (one RCCL all-gather of latent tiles + one gather of pixel tiles).
"""
import math
import os
import threading
import time
from argparse import ArgumentParser, Namespace
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, Iterable, Iterator, List

import numpy as np
import torch
from PIL import Image

DEFAULT_PROMPT = ("./output/tmp/real-world image, realistic, high quality, photograph, film, professional, 4k, "
                  "highly detailed_300token.pth")


def parse_args() -> Namespace:
    parser = ArgumentParser()
    parser.add_argument("--ckpt", required=True, type=str, help="full checkpoint path", default="./weights/InstaRevive_v1.ckpt")
    parser.add_argument("--input", type=str, required=True)
    parser.add_argument("--sr_scale", type=float, default=1)
    parser.add_argument("--repeat_times", type=int, default=1)
    parser.add_argument("--disable_preprocess_model", action="store_true")
    # patch-based sampling
    parser.add_argument("--tiled", action="store_true")
    parser.add_argument("--tile_size", type=int, default=512)
    parser.add_argument("--tile_stride", type=int, default=448)
    # latent image guidance (accepted and inert, like the reference)
    parser.add_argument("--use_guidance", action="store_true")
    parser.add_argument("--g_scale", type=float, default=0.0)
    parser.add_argument("--g_t_start", type=int, default=1001)
    parser.add_argument("--g_t_stop", type=int, default=-1)
    parser.add_argument("--g_space", type=str, default="latent")
    parser.add_argument("--g_repeat", type=int, default=5)
    parser.add_argument("--color_fix_type", type=str, default="wavelet", choices=["wavelet", "adain", "none"])
    parser.add_argument("--output", type=str, required=True)
    parser.add_argument("--show_lq", action="store_true")
    parser.add_argument("--skip_if_exist", action="store_true")
    parser.add_argument("--seed", type=int, default=231)
    parser.add_argument("--device", type=str, default="cuda", choices=["cpu", "cuda", "mps"])
    parser.add_argument("--use_prompt", action="store_true")
    parser.add_argument("--use_center_crop", action="store_true")
    # locations the reference hard-codes
    parser.add_argument("--swinir_ckpt", type=str, default="./weights/general_swinir_v1.ckpt")
    parser.add_argument("--swinir_config", type=str, default="./configs/swinir.yaml")
    parser.add_argument("--vae", type=str, default="stabilityai/sd-vae-ft-ema")
    parser.add_argument("--dit_config", type=str, default="PixArt-alpha/PixArt-Alpha-DMD-XL-2-512x512")
    parser.add_argument("--prompt_embeds", type=str, default=DEFAULT_PROMPT)
    parser.add_argument("--caption_dir", type=str, default=None, help="per-image prompts (no reference flag: the evaluation loop's captions, "
                        "test_dmd_general.py:173-174): DIR/<input-relative path without extension>.npz, else DIR/<file stem>.npz (caption_feature "
                        "[1, T, 4096], optional attention_mask). Images without one get --prompt_embeds; every prompt needs the same T")
    add_text_prompt_flags(parser)
    # extensions (defaults reproduce the reference's behaviour)
    parser.add_argument("--batch_size", type=int, default=1, help="consecutive files of equal network-input size per process() call")
    parser.add_argument("--shard_tiles", action="store_true", help="with --tiled under torchrun: spread the TILES of each image over the "
                        "GPUs (one large image at a time) instead of spreading the files")
    parser.add_argument("--fp8", type=str, default="off", choices=["off", "default", "auto", "qualified", "all", "attention"], help="BASELINE.json configs[4]: fp8 (e4m3) MFMA "
                        "operands. default (= auto): the operand set is chosen ON THE LOADED WEIGHTS at start-up - one 512 x 512 calibration image, every part alone "
                        "against the bf16 pass (about a second; cached per weight set) - so that the result stays within 0.1 dB PSNR of the bf16 / reference path up to a "
                        "30 dB reference: on flat-softmax weights that is the attention products + two decoder conv levels (about 15 %% faster), on weights with "
                        "heavy-tailed channels / peaky attention fewer parts or none (instarevive_amd/fp8_select.py). qualified = that flat-softmax set without "
                        "calibration; attention = the attention products only; all = every part (about 22 %% faster, 42 dB against the reference path: out of the "
                        "tolerance). off is the default")
    parser.add_argument("--png_compress_level", type=int, default=None, choices=range(0, 10), metavar="0..9", help="zlib level of the saved PNGs; default: PIL's own "
                        "(6, what the reference writes). The pixels are the same at every level; 1 costs about a third of the encoder time - for ranks whose CPU share "
                        "cannot keep up with the GPU (the CLI says so at start-up)")
    parser.add_argument("--png_encoder", type=str, default="host", choices=["host", "gpu"], help="who compresses the saved PNGs. host (default): PIL / zlib on the "
                        "writer threads, as the reference does. gpu: the device encodes the result behind the network (Paeth filter + Huffman coding of literals, no "
                        "LZ77 matches; lossless, the same pixels) and only the compressed bytes cross PCIe - for restored PHOTOGRAPHS, where its files are 10 - 18 %% "
                        "smaller than --png_compress_level 1 and within a few percent of the default level; flat or near-flat content (smooth sky, graphics) comes "
                        "out several times larger than PIL's, since a byte never costs less than one bit (--png_runs lifts that). Files that are not a plain crop of the prediction "
                        "(--show_lq; inputs that auto_resize enlarged, unless --resize gpu resizes their results on the device) still take the host encoder; the run says how many")
    parser.add_argument("--png_runs", action="store_true", help="with --png_encoder gpu: the device encoder's run mode (ir_png_encode_runs). Runs of equal "
                        "filtered bytes are coded as matches at distance 1 and the block headers are compacted, chunk by chunk wherever that is shorter: the same "
                        "pixels, no file larger than without the flag, flat content (sky, graphics) 6 - 35 times smaller (1.6 - 1.9 times PIL's default level, "
                        "about PIL's level 1), sky over a photograph 1.29 times smaller and below PIL's default (sizes of the format's CPU model on 512 x 512 "
                        "cases, docs/parity.md). Measured: the encode then takes 0.72 ms instead of 0.38 ms per 2048 x 2048 result, 0.61 %% of the step "
                        "(profiles/png_runs.txt). The default mode is unchanged")
    add_jpeg_flags(parser)
    parser.add_argument("--resize", type=str, default="host", choices=["host", "gpu"], help="who resizes the inputs (--sr_scale and the enlargement of short edges "
                        "below 512 / the tile size, both bicubic) and the results of enlarged inputs (LANCZOS back to the input's size). host (default): PIL on the "
                        "reader / writer threads, as the reference does. gpu: the decoded file is uploaded as it is and the device resamples it with Pillow's own "
                        "integer arithmetic - the same pixels in the saved files - so the enlarged image neither costs a reader thread its bicubic nor crosses "
                        "PCIe, and with --png_encoder gpu every file is encoded on the device. --show_lq, --use_center_crop (unless --center_crop gpu makes the crop on the device too) and --shard_tiles keep "
                        "the host path")
    parser.add_argument("--gt", type=str, default=None, help="score the results against ground truth on the GPU (PSNR-Y / SSIM-Y by the definitions of "
                        "tools/evaluate_pairs.py, i.e. pyiqa's): DIR/<input-relative path> with any image extension, else DIR/<file stem>.*; a ground truth has the "
                        "size of the saved result. A file is scored when its saved image is the device's image - a plain crop of the prediction, and every file "
                        "under --resize gpu; the run says how many were not (inputs the host enlarged, --show_lq). Not offered with --shard_tiles")
    parser.add_argument("--metrics_out", type=str, default=None, help="with --gt: the CSV of per-file scores (file,psnr_y,ssim_y); default <output>/metrics.csv, "
                        "metrics.rank<k>.csv with several ranks. Each rank prints the averages of its own files")
    parser.add_argument("--lpips_lin", type=str, default=None, help="with --gt: score LPIPS (v0.1, alex) on the GPU as well (ir_lpips, exact fp32). FILE holds the "
                        "lpips linear heads (lpips/weights/v0.1/alex.pth) or a full lpips.LPIPS() state dict, as tools/evaluate_pairs.py takes them. The CSV "
                        "becomes file,psnr_y,ssim_y,lpips and the averages gain `lpips: x.xxxxx`; every scored image needs 31 x 31 pixels")
    parser.add_argument("--lpips_alexnet", type=str, default=None, help="with --lpips_lin holding the heads alone: torchvision's AlexNet state dict "
                        "(alexnet-owt-7be5be79.pth)")
    parser.add_argument("--dists_model", type=str, default=None, metavar="FILE", help="with --gt (or --degrade): score DISTS on the GPU as well (ir_dists: VGG-16 at the "
                        "image's own size in exact fp32, fp64 statistics; the definition of tools/evaluate_pairs.py::DISTS, i.e. pyiqa's `dists` defaults). FILE is "
                        "one state dict in the DISTS module's names, or alpha / beta alone (DISTS_weights.pt) together with --dists_vgg, or an .npz in "
                        "ir_dists_configure's names. The CSV gains the column `dists` and the averages `dists: x.xxxxx`, both last. Which files are scored follows "
                        "--gt's rule; files below 16 x 16 pixels are counted as not scored. Opt-in: the thirteen convolutions at full size cost about as much as "
                        "the network itself. Not offered with --shard_tiles")
    parser.add_argument("--dists_vgg", type=str, default=None, metavar="FILE", help="with --dists_model holding alpha / beta alone: torchvision's VGG-16 state dict "
                        "(vgg16-397923af.pth)")
    parser.add_argument("--fid_model", type=str, default=None, metavar="FILE", help="FID of the run's results on the GPU (ir_fid_features: pytorch-fid's Inception-v3 in "
                        "exact fp32 on every saved result, the Frechet distance in fp64 at the end of the run; the definition of tools/evaluate_fid.py). FILE is "
                        "pytorch-fid's pt_inception state dict or an .npz in ir_fid_configure's names. The reference set is the ground truth of the scored "
                        "files (--gt or --degrade) or --fid_stats; with neither the flag is refused. The averages gain one last line `fid: x.xxxxx`; metrics.csv "
                        "does not change (FID has no per-file value). Which files enter the set follows --gt's rule (the saved image is the device's image); "
                        "the run prints both counts. Opt-in. Not offered with --shard_tiles")
    parser.add_argument("--fid_resize", type=str, default="clean", choices=["clean", "legacy"], help="with --fid_model: how an image becomes the 299 x 299 input: clean "
                        "(pyiqa's fid, clean-fid: Pillow's float BICUBIC, antialiased) or legacy (pytorch-fid: torch's bilinear)")
    parser.add_argument("--fid_stats", type=str, default=None, metavar="FILE.npz", help="with --fid_model: the reference set's statistics (pytorch-fid's mu / sigma); needs no --gt")
    parser.add_argument("--fid_features_out", type=str, default=None, metavar="FILE", help="with --fid_model: where the features of the run go (default "
                        "<output>/fid_features.npz; with several ranks fid_features.rank<k>.npz, which rank 0 merges)")
    parser.add_argument("--niqe_params", type=str, default=None, help="score NIQE, the no-reference metric of the reference's evaluate_img.py that is no "
                        "pretrained network, on the GPU (ir_niqe_stats; the definition of tools/evaluate_niqe.py, i.e. pyiqa's defaults). FILE holds the pristine "
                        "parameters mu_prisparam [36] / cov_prisparam [36][36]: pyiqa's niqe_modelparameters.mat, or an .npz. Works without --gt: the CSV is then "
                        "file,niqe and the average prints as `niqe: x.xxxxx`; with --gt the column and the line come last. Which files are scored follows --gt's "
                        "rule (the saved image is the device's image); files below 96 pixels on an edge or without two complete feature rows are counted as not scored")
    parser.add_argument("--ilniqe_params", type=str, default=None, help="score IL-NIQE, the no-reference metric the reference's evaluate_img.py keeps commented out "
                        "next to niqe, on the GPU (ir_ilniqe_stats; the definition of tools/evaluate_ilniqe.py). FILE is the user's ILNIQE_templateModel.mat, or an "
                        ".npz with mu_prisparam / cov_prisparam / meanOfSampleData / principleVectors. Works with or without --gt and the other metric flags: the "
                        "column `ilniqe` stands right behind niqe's place and the average prints as `ilniqe: x.xxxxx`. Which files are scored follows --gt's rule")
    parser.add_argument("--clipiqa_model", type=str, default=None, help="score CLIP-IQA, the no-reference metric `clipiqa` of the reference's evaluate_img.py, on "
                        "the GPU (ir_clipiqa; the definition of tools/evaluate_clipiqa.py, i.e. pyiqa's default over OpenAI CLIP RN50 at the image's own size). "
                        "FILE is OpenAI's RN50.pt (TorchScript archive or state dict), or an .npz with the same names - which may carry the ten text rows as "
                        "`text`, so that no vocabulary is needed. Works with or without --gt and --niqe_params: the column `clipiqa` and the line "
                        "`clipiqa: x.xxxxx` come last. Which files are scored follows --gt's rule; files below 32 pixels on an edge are counted as not scored")
    parser.add_argument("--musiq_model", type=str, default=None, help="score MUSIQ, the no-reference metric `musiq` of the reference's evaluate_img.py, on the "
                        "GPU (ir_musiq; the definition of tools/evaluate_musiq.py, i.e. pyiqa's default koniq10k configuration, in exact fp32). FILE is an "
                        ".npz in that file's names, or pyiqa's .pth state dict. Works with or without --gt, --niqe_params and --clipiqa_model: the column "
                        "`musiq` and the line `musiq: x.xxxxx` come last. Which files are scored follows --gt's rule; files of which a resized side rounds "
                        "to 0 (1 x 1000) are counted as not scored")
    parser.add_argument("--maniqa_model", type=str, default=None, help="score MANIQA, the no-reference metric `maniqa` of the reference's evaluate_img.py, on the "
                        "GPU (ir_maniqa; the definition of tools/evaluate_maniqa.py, i.e. pyiqa's koniq configuration, in exact fp32). FILE is an "
                        ".npz in that file's names, or pyiqa's .pth state dict. Works with or without --gt and the other scorers: the column "
                        "`maniqa` and the line `maniqa: x.xxxxx` come last. Which files are scored follows --gt's rule; files with a short side of "
                        "224 or less are counted as not scored. Costs about as much as the network's own step (20 crops through a ViT-B/8)")
    parser.add_argument("--topiq_model", type=str, default=None, help="score TOPIQ-NR, the no-reference metric `topiq_nr` that the reference's evaluate_img.py names, on the "
                        "GPU (ir_topiq; the definition of tools/evaluate_topiq.py, i.e. pyiqa's CFANet with a ResNet-50 trunk at the image's own size, in exact "
                        "fp32). FILE is an .npz in that file's names, or pyiqa's .pth state dict. Works with or without --gt and the other scorers: the column "
                        "`topiq_nr` and the line `topiq_nr: x.xxxxx` come behind maniqa's and before dists's. Which files are scored follows --gt's rule; "
                        "files with a side below 16 are counted as not scored. Not offered with --shard_tiles")
    parser.add_argument("--maniqa_crops", type=str, default="uniform", choices=["uniform", "random"], help="with --maniqa_model: where the 20 crops lie. uniform "
                        "(default): pyiqa's grid. random: drawn from --maniqa_seed and the saved file's name (as tools/evaluate_maniqa.py draws them for that file), whatever the batch size, worker "
                        "count or rank")
    parser.add_argument("--maniqa_seed", type=int, default=None, help="with --maniqa_crops random: the seed (default 231)")
    parser.add_argument("--clip_bpe", type=str, default=None, help="with --clipiqa_model: the folder that holds CLIP's BPE table (bpe_simple_vocab_16e6.txt.gz, or "
                        "vocab.json + merges.txt), from which the ten prompts are tokenised")
    parser.add_argument("--degrade", type=str, nargs="?", const="lq", default=None, metavar="lq|realesrgan|FILE.json", help="--input holds GROUND TRUTH: synthesise every "
                        "file's low-quality image on the GPU (ir_degrade; the definition of tools/degrade_folder.py) and restore that - the first-order "
                        "degradation of the reference's dataset/codeformer.py and tools/lq.py: 41 x 41 iso / aniso Gaussian blur, bilinear downsample by "
                        "U[2,4], Gaussian noise of sigma U[0,20], JPEG at quality int(U[60,100]), bilinear resize back. `lq` (default) holds tools/lq.py's "
                        "constants; a JSON file may set blur_kernel_size, kernel_list (iso, aniso), kernel_prob, blur_sigma, downsample_range, noise_range, "
                        "jpeg_range and norm (none, or max for tools/lq.py's division by the maximum). `realesrgan` is the SECOND-ORDER recipe the reference "
                        "validates general super-resolution with (configs/general_deg_realesrgan_val.yaml; ir_degrade_chain): two stages of blur, area / "
                        "bilinear / bicubic resize, Gaussian or Poisson noise and DiffJPEG, a final sinc filter, bicubic back - files of at least 44 pixels "
                        "on the short side; a JSON file with \"chain\": \"realesrgan\" may set that recipe's keys. No OpenCV, no second folder: the LQ image never "
                        "leaves the device. Switches --resize gpu on; not offered with --show_lq, --use_center_crop (unless --center_crop gpu), --shard_tiles. Without --gt the input "
                        "folder is the ground truth of --metrics_out / --lpips_lin / --niqe_params / --clipiqa_model / --musiq_model / --maniqa_model")
    parser.add_argument("--degrade_seed", type=int, default=231, help="with --degrade: a file's parameters are drawn from a generator seeded by this number "
                        "and the crc32 of its input-relative path, whatever the batch size, worker count or rank")
    parser.add_argument("--save_lq", type=str, default=None, metavar="DIR", help="with --degrade: write the synthesised LQ images to DIR/<input-relative path>.png")
    parser.add_argument("--jpeg_decoder", type=str, default="host", choices=["host", "gpu"], help="who decodes JPEG inputs. host (default): PIL, as the reference. gpu: "
                        "a reader thread parses the headers and removes the byte stuffing, the compressed bytes are uploaded and ir_jpeg_decode makes PIL's "
                        "pixels on the device (baseline files, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0; every other file, JPEG or not, takes PIL as today and the "
                        "run says how many). Switches --resize gpu on; not offered with --show_lq, --use_center_crop (unless --center_crop gpu), --shard_tiles")
    parser.add_argument("--png_decoder", type=str, default="host", choices=["host", "gpu"], help="who decodes PNG inputs. host (default): PIL, as the reference. gpu: "
                        "a reader thread walks the chunks and checks their CRCs, the compressed bytes are uploaded and ir_png_decode inflates, unfilters and "
                        "converts on the device to PIL's pixels (8 bits a sample, grey / RGB with or without alpha, not interlaced; every other file, PNG or "
                        "not, takes PIL as today and the run says how many). May be given together with --jpeg_decoder gpu. Switches --resize gpu on; not "
                        "offered with --show_lq, --use_center_crop (unless --center_crop gpu), --shard_tiles")
    parser.add_argument("--center_crop", type=str, default="host", choices=["host", "gpu"], help="who makes the centre crop of --use_center_crop. host (default): PIL on a "
                        "reader thread, as the reference does (center_crop_arr: BOX halvings, a bicubic resize of the short edge to 512, the central window). gpu: "
                        "the decoded file - or, with --jpeg_decoder gpu, its compressed bytes - is uploaded and the device runs the same chain with Pillow's own "
                        "integer arithmetic (ir_resample_u8 with BOX plans, ir_resample_u8_window for the last step): the same pixels in the network input. Needs "
                        "--use_center_crop and switches --resize gpu on; with it --use_center_crop is accepted next to --jpeg_decoder gpu and --degrade (the crop "
                        "is then what is degraded). Not offered with --tiled, --show_lq, --shard_tiles")
    parser.add_argument("--workers", type=int, default=-1, help="host threads that decode / resize the inputs and resize / PNG-encode the results "
                        "around the GPU (PIL releases the GIL there); -1 = this process's CPU share, 0 = everything on the main thread like the reference")
    return parser.parse_args()


def add_text_prompt_flags(parser) -> None:
    """--prompt, --captions and what goes with them (eval_batch.py takes the same ones): prompts as text, T5-encoded inside the run."""
    from instarevive_amd.text_prompts import add_flags
    add_flags(parser)


def check_text_prompts(args: Namespace) -> None:
    """The refusals around --prompt / --captions, one line each; before anything is loaded."""
    from instarevive_amd.text_prompts import check_flags
    msg = check_flags(args, DEFAULT_PROMPT)
    if msg:
        raise SystemExit(msg)


def add_jpeg_flags(parser) -> None:
    """--save_format and the --jpeg_* flags (eval_batch.py takes the same ones). The --jpeg_* defaults are None until check_save_format() has
    seen whether they were given."""
    parser.add_argument("--save_format", type=str, default="png", choices=["png", "jpg"], help="the format of the saved results. png (default): lossless, what the "
                        "reference writes. jpg: baseline JPEG (standard Huffman tables, JFIF, no other metadata), the save path then ends in .jpg - a 2048 x 2048 "
                        "result takes 1 - 2 MB instead of 8 - 12. Scoring (--gt, --niqe_params, --clipiqa_model, --musiq_model, --maniqa_model) still reads the device's image, the result "
                        "BEFORE the JPEG loss")
    parser.add_argument("--jpeg_quality", type=int, default=None, metavar="1..100", help="with --save_format jpg: libjpeg's quality (default 95)")
    parser.add_argument("--jpeg_subsampling", type=str, default=None, choices=["420", "444"], help="with --save_format jpg: chroma subsampling, 420 (default) or 444")
    parser.add_argument("--jpeg_encoder", type=str, default=None, choices=["host", "gpu"], help="with --save_format jpg: who codes the files. host (default): PIL / "
                        "libjpeg on the writer threads. gpu: the device codes the result behind the network (ir_jpeg_encode) and only the coded bytes cross PCIe. "
                        "The files are the same bytes either way. Files whose saved image is not the device's image (--show_lq; inputs that auto_resize "
                        "enlarged, unless --resize gpu resizes their results on the device; --use_center_crop next to --tiled; --shard_tiles) take the host "
                        "encoder; the run says how many")


def check_save_format(args: Namespace) -> None:
    """The refusals around --save_format and the PNG encoder's flags, one line each, and the --jpeg_* defaults; before anything is loaded."""
    if getattr(args, "png_runs", False) and getattr(args, "png_encoder", "host") != "gpu":
        raise SystemExit("--png_runs is the run mode of the device PNG encoder: give --png_encoder gpu as well")
    given = [f"--{k}" for k in ("jpeg_quality", "jpeg_subsampling", "jpeg_encoder") if getattr(args, k, None) is not None]
    if args.save_format != "jpg":
        if given:
            raise SystemExit(f"{' / '.join(given)} set how JPEGs are written: give --save_format jpg as well")
        args.jpeg_encoder = "host"
        return
    if getattr(args, "png_encoder", "host") == "gpu" or getattr(args, "png_compress_level", None) is not None:
        raise SystemExit("--png_encoder gpu / --png_compress_level set how PNGs are written: not offered together with --save_format jpg")
    args.jpeg_quality = 95 if args.jpeg_quality is None else args.jpeg_quality
    if not 1 <= args.jpeg_quality <= 100:
        raise SystemExit(f"--jpeg_quality {args.jpeg_quality} is outside 1 .. 100")
    args.jpeg_subsampling = args.jpeg_subsampling or "420"
    args.jpeg_encoder = args.jpeg_encoder or "host"


def crop_on_gpu(args: Namespace) -> bool:
    """--center_crop gpu (a Namespace without the attribute is the host crop of before the flag)."""
    return getattr(args, "center_crop", "host") == "gpu"


def check_center_crop(args: Namespace) -> None:
    """--center_crop gpu makes --use_center_crop's crop on the device's resize route: it switches --resize gpu on and is refused where that route
    is not offered. One line each, before anything is loaded."""
    if not crop_on_gpu(args):
        return
    if not getattr(args, "use_center_crop", False):
        raise SystemExit("--center_crop gpu says who makes the crop of --use_center_crop: give --use_center_crop as well")
    for flag in ("tiled", "show_lq", "shard_tiles"):
        if getattr(args, flag, False):
            raise SystemExit(f"--center_crop gpu crops on the device's resize route (--resize gpu), which is not offered with --{flag}: not offered together")
    if args.resize != "gpu":
        print("--center_crop gpu: the crops are made on the device, switching --resize gpu on")
        args.resize = "gpu"


def check_jpeg_decoder(args: Namespace) -> None:
    """--jpeg_decoder gpu decodes into the device's resize route: it switches --resize gpu on and is refused wherever that is."""
    if getattr(args, "jpeg_decoder", "host") != "gpu":
        return
    for flag in ("show_lq", "use_center_crop", "shard_tiles"):
        if getattr(args, flag, False) and not (flag == "use_center_crop" and crop_on_gpu(args)):
            raise SystemExit(f"--jpeg_decoder gpu decodes into the device's resize route (--resize gpu), which --{flag} keeps on the host: not offered together"
                             + (" (or give --center_crop gpu)" if flag == "use_center_crop" else ""))
    if args.resize != "gpu":
        print("--jpeg_decoder gpu: the files are decoded on the device, switching --resize gpu on")
        args.resize = "gpu"
    args.jpeg_decode_log = []   # per file None (decoded on the device) or the reason it took the host decoder; list.append is atomic


def jpeg_decoder_note(args: Namespace) -> str:
    log = getattr(args, "jpeg_decode_log", None)
    if log is None:
        return ""
    host = [r for r in log if r is not None]
    reasons = ", ".join(f"{r}: {host.count(r)}" for r in sorted(set(host)))
    return (f"--jpeg_decoder gpu: {len(log) - len(host)} of {len(log)} files were decoded on the device, {len(host)} took the host decoder"
            + (f" (reasons: {reasons})" if host else ""))


def check_png_decoder(args: Namespace) -> None:
    """--png_decoder gpu decodes into the device's resize route, as --jpeg_decoder gpu does: it switches --resize gpu on and makes the same refusals."""
    if getattr(args, "png_decoder", "host") != "gpu":
        return
    for flag in ("show_lq", "use_center_crop", "shard_tiles"):
        if getattr(args, flag, False) and not (flag == "use_center_crop" and crop_on_gpu(args)):
            raise SystemExit(f"--png_decoder gpu decodes into the device's resize route (--resize gpu), which --{flag} keeps on the host: not offered together"
                             + (" (or give --center_crop gpu)" if flag == "use_center_crop" else ""))
    if args.resize != "gpu":
        print("--png_decoder gpu: the files are decoded on the device, switching --resize gpu on")
        args.resize = "gpu"
    args.png_decode_log = []   # per file None (decoded on the device) or the reason it took the host decoder; list.append is atomic


def png_decoder_note(args: Namespace) -> str:
    log = getattr(args, "png_decode_log", None)
    if log is None:
        return ""
    host = [r for r in log if r is not None]
    reasons = ", ".join(f"{r}: {host.count(r)}" for r in sorted(set(host)))
    return (f"--png_decoder gpu: {len(log) - len(host)} of {len(log)} files were decoded on the device, {len(host)} took the host decoder"
            + (f" (reasons: {reasons})" if host else ""))


def device_source(file_path: str, args: Namespace):
    """--jpeg_decoder gpu / --png_decoder gpu: the file as a JpegSource or PngSource (the headers and one pass over the bytes, on a reader thread), or
    None for a file that takes PIL; the reason goes to the flag's log. With both flags a file with PNG's signature is the PNG decoder's, every
    other one the JPEG decoder's."""
    jlog, plog = getattr(args, "jpeg_decode_log", None), getattr(args, "png_decode_log", None)
    if jlog is None and plog is None:
        return None
    with open(file_path, "rb") as f:
        data = f.read()
    if plog is not None and (jlog is None or data[:8] == b"\x89PNG\r\n\x1a\n"):
        from instarevive_amd.png_decode import PngSource
        source, why = PngSource.open(data)
        plog.append(why)
    else:
        from instarevive_amd.jpeg_decode import JpegSource
        source, why = JpegSource.open(data)
        jlog.append(why)
    if source is not None:
        source.name = file_path
    return source


def save_ext(args: Namespace) -> str:
    return ".jpg" if getattr(args, "save_format", "png") == "jpg" else ".png"


def cpu_share() -> int:
    """Cores this process may really use: the affinity mask, cut down to the cgroup's CPU quota when one is set (a GPU box hands each job a
    share - 16 cores per GPU - of a host whose affinity mask still shows every core; PNG encoders beyond the quota only time-slice against
    the thread that launches the kernels)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: t.split()), ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: [t.strip(), None])):
        try:
            with open(path) as f:
                quota, period = parse(f.read())
            if period is None:
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                    period = f.read().strip()
            if quota not in ("max", "-1") and int(quota) > 0 and int(period) > 0:
                cores = min(cores, max(1, int(quota) // int(period)))
            break
        except (OSError, ValueError):
            continue
    return cores


def default_workers(local_world: int = 1) -> int:
    """Host threads for this rank: its part of the CPU share, less the cores kept for the thread that feeds the GPU and the copy engine's callbacks
    (two; one when the rank's part is 8 cores or fewer - 8 ranks on a 64-core host - where the feeding thread, asleep in stream waits most of the time,
    shares a core with an encoder rather than take a quarter of the rank's budget), at most 16 (one MI355X produces ~8 results of 2048 x 2048 a second and
    a PNG of that size costs 0.8 - 1.7 core-seconds on the host encoder, which is what this count is sized for; under --png_encoder gpu a file costs the host about
    0.03 core-seconds, paid on the writer threads (the feeding thread only copies the compressed bytes out of the pinned buffer), and two or three threads would do - the count is not lowered for it, since files that are not plain crops still take the host encoder (without --resize gpu: every input that auto_resize enlarged);
    $IR_WORKERS overrides)."""
    if os.environ.get("IR_WORKERS"):
        return max(0, int(os.environ["IR_WORKERS"]))
    part = cpu_share() // max(local_world, 1)
    return max(1, min(16, part - (2 if part > 8 else 1)))


PNG_CORE_SECONDS_2048 = 1.25   # PIL's default encoder (compress_level 6) on one 2048 x 2048 RGB result: 0.8 - 1.7 core-seconds by content (profiles/r05_cli_rate_ab.txt)
PNG_GPU_HOST_CORE_SECONDS_2048 = 0.03   # --png_encoder gpu: what is left to the host per 2048 x 2048 result - one CRC-32 over ~8 MB of compressed bytes (10 ms), the copies into the file's bytes and the write
GPU_FILES_PER_SECOND_2048 = 8.4   # what one MI355X delivers at 2048 x 2048 (bench.py `value`)


def host_keeps_up(workers: int, out_pixels: int, compress_level, encoder: str = "host") -> str:
    """'' when `workers` encoder threads keep ahead of one GPU for results of out_pixels pixels, else the sentence the CLI prints: the rank is then
    host-bound (8 ranks on a 64-core host: 7 threads encode ~5.6 files/s of 2048 x 2048 at PIL's default level against ~8.4 from the GPU). The estimate
    scales the measured level-6 cost by the pixel count; level 1 costs about a third of it (larger files, the same pixels). encoder = "gpu" prices a
    file at the host's share of the device encoder (PNG_GPU_HOST_CORE_SECONDS_2048), for runs whose files are plain crops of the prediction or, under --resize gpu, resized on the device."""
    if workers <= 0 or out_pixels <= 0:
        return ""
    scale = out_pixels / float(2048 * 2048)
    cost = PNG_CORE_SECONDS_2048 * scale * (1.0 if compress_level is None or compress_level >= 6 else (0.35 if compress_level <= 1 else 0.6))
    if encoder == "gpu":
        cost = PNG_GPU_HOST_CORE_SECONDS_2048 * scale
    host_rate, gpu_rate = workers / cost, GPU_FILES_PER_SECOND_2048 / scale
    if host_rate >= gpu_rate:
        return ""
    return (f"host-bound: {workers} encoder threads write ~{host_rate:.1f} files/s of {out_pixels / 1e6:.1f} Mpixel against ~{gpu_rate:.1f} from the GPU - give the rank more "
            f"cores (--workers / $IR_WORKERS), or trade file size for speed with --png_compress_level 1 (same pixels, lossless)"
            + ("" if encoder == "gpu" else ", or encode photographs on the GPU with --png_encoder gpu"))


def load_ilniqe_params(args: Namespace):
    """--ilniqe_params: the template, read before any model is touched; a file that is missing or holds anything else ends the run."""
    if not getattr(args, "ilniqe_params", None):
        return None
    from instarevive_amd.ilniqe import IlniqeError, load_params
    if not os.path.isfile(args.ilniqe_params):
        raise SystemExit(f"--ilniqe_params {args.ilniqe_params}: no such file")
    try:
        return load_params(args.ilniqe_params)
    except IlniqeError as e:
        raise SystemExit(str(e))


def load_niqe_params(args: Namespace):
    """--niqe_params: the pristine parameters, read before any model is touched; a file that is missing or holds anything else ends the run."""
    if not getattr(args, "niqe_params", None):
        return None
    from instarevive_amd.niqe import NiqeError, load_params
    if not os.path.isfile(args.niqe_params):
        raise SystemExit(f"--niqe_params {args.niqe_params}: no such file")
    try:
        return load_params(args.niqe_params)
    except NiqeError as e:
        raise SystemExit(str(e))


def load_clipiqa_model(args: Namespace):
    """--clipiqa_model [--clip_bpe]: the CLIP-IQA model with its text rows, read before any other model is touched; a file that is missing or holds
    anything else ends the run."""
    if not getattr(args, "clipiqa_model", None):
        if getattr(args, "clip_bpe", None):
            raise SystemExit("--clip_bpe needs --clipiqa_model")
        return None
    from instarevive_amd import clipiqa
    if not os.path.isfile(args.clipiqa_model):
        raise SystemExit(f"--clipiqa_model {args.clipiqa_model}: no such file")
    try:
        return clipiqa.load_model(args.clipiqa_model, args.clip_bpe)
    except (ValueError, FileNotFoundError) as e:   # ClipIqaError is a ValueError
        raise SystemExit(f"--clipiqa_model {args.clipiqa_model}: {e}")


def load_musiq_model(args: Namespace):
    """--musiq_model: the MUSIQ model, read before any other model is touched; a file that is missing or holds anything else ends the run."""
    if not getattr(args, "musiq_model", None):
        return None
    from instarevive_amd import musiq
    if not os.path.isfile(args.musiq_model):
        raise SystemExit(f"--musiq_model {args.musiq_model}: no such file")
    try:
        return musiq.load_model(args.musiq_model)
    except Exception as e:   # MusiqError is a ValueError; a file torch cannot unpickle raises its own kinds
        raise SystemExit(f"--musiq_model {args.musiq_model}: {e}")


def load_maniqa_model(args: Namespace):
    """--maniqa_model: the MANIQA model, read before any other model is touched; a file that is missing or holds anything else ends the run.
    --maniqa_crops random without --maniqa_seed takes the stated default seed."""
    if not getattr(args, "maniqa_model", None):
        if getattr(args, "maniqa_seed", None) is not None or getattr(args, "maniqa_crops", "uniform") != "uniform":
            raise SystemExit("--maniqa_crops / --maniqa_seed need --maniqa_model")
        return None
    from instarevive_amd import maniqa
    if args.maniqa_crops != "random" and args.maniqa_seed is not None:
        raise SystemExit("--maniqa_seed seeds --maniqa_crops random: give that as well")
    if args.maniqa_crops == "random" and args.maniqa_seed is None:
        args.maniqa_seed = maniqa.DEFAULT_SEED
    if not os.path.isfile(args.maniqa_model):
        raise SystemExit(f"--maniqa_model {args.maniqa_model}: no such file")
    try:
        return maniqa.load_model(args.maniqa_model)
    except Exception as e:   # ManiqaError is a ValueError; a file torch cannot unpickle raises its own kinds
        raise SystemExit(f"--maniqa_model {args.maniqa_model}: {e}")


def load_topiq_model(args: Namespace):
    """--topiq_model: the TOPIQ-NR model, read before any other model is touched; a file that is missing or holds anything else ends the run with the
    loader's message. Not offered with --shard_tiles."""
    if not getattr(args, "topiq_model", None):
        return None
    if getattr(args, "shard_tiles", False):
        raise SystemExit("--topiq_model is not offered together with --shard_tiles (the assembled frame of the tile-sharded path is not scored on the device)")
    from instarevive_amd import topiq
    if not os.path.isfile(args.topiq_model):
        raise SystemExit(f"--topiq_model {args.topiq_model}: no such file")
    try:
        return topiq.load_model(args.topiq_model)
    except Exception as e:   # TopiqError is a ValueError; a file torch cannot unpickle raises its own kinds
        raise SystemExit(f"--topiq_model {args.topiq_model}: {e}")


def load_dists_weights(args: Namespace):
    """--dists_model [--dists_vgg]: the tensors ir_dists_configure binds, read before any other model is touched. The flag alone (no --gt, no
    --degrade), with --shard_tiles, or with a file that is missing or holds anything else ends the run in one line."""
    if not getattr(args, "dists_model", None):
        if getattr(args, "dists_vgg", None):
            raise SystemExit("--dists_vgg needs --dists_model (DISTS' alpha / beta)")
        return None
    if not (getattr(args, "gt", None) or getattr(args, "degrade", None)):
        raise SystemExit("--dists_model scores against ground truth: give --gt (or --degrade) as well")
    if getattr(args, "shard_tiles", False):
        raise SystemExit("--dists_model is not offered together with --shard_tiles (the assembled frame of the tile-sharded path is not scored on the device)")
    for flag in ("dists_model", "dists_vgg"):
        if getattr(args, flag, None) and not os.path.isfile(getattr(args, flag)):
            raise SystemExit(f"--{flag} {getattr(args, flag)}: no such file")
    from instarevive_amd import dists
    try:
        return dists.load_weights(args.dists_model, args.dists_vgg)
    except Exception as e:   # KeyError / ValueError of the loader; a file torch cannot unpickle raises its own kinds
        raise SystemExit(f"--dists_model {args.dists_model}: {e}")


def load_fid(args: Namespace):
    """--fid_model [--fid_stats]: (the tensors ir_fid_configure binds, the reference statistics or None), read before any other model is touched;
    (None, None) without the flag. The refusals are fid.check_flags'."""
    if not any(getattr(args, f, None) for f in ("fid_model", "fid_stats", "fid_features_out")) and getattr(args, "fid_resize", "clean") == "clean":
        return None, None
    from instarevive_amd import fid
    return fid.check_flags(args, bool(getattr(args, "gt", None) or getattr(args, "degrade", None)))


def check_device(device: str) -> str:
    if device != "cuda" or not torch.cuda.is_available():
        raise SystemExit(f"device '{device}' requested / no GPU visible: this build runs on MI355X (ROCm) only and has no CPU or MPS path")
    print(f"using device {device}")
    return device


# ---------------------------------------------------------------------------------------------------------------------
# The reference runs one file at a time through load -> resize -> pad -> process() -> crop -> resize -> save, all on one host thread
# (test_scripts/inference.py:261-346). Here the same per-file arithmetic is cut into three pieces around the GPU call:
#   read_job()    everything before process(): decode, --sr_scale bicubic, auto_resize / centre crop, pad to 64       (:263-291)
#   process_stream()  the GPU path, transfers of neighbouring jobs overlapped with compute
#   write_job()   everything after: un-pad, LANCZOS back to the LQ size, optional LQ | stage-1 | result strip, PNG    (:323-346)
# so that a directory streams through the GPU instead of alternating between PIL and the device.
@dataclass
class Job:
    save_path: str
    lq: Image.Image            # the (sr_scale-d) LQ image: target size of the saved result and left panel of --show_lq
    net_in: np.ndarray         # what process() receives: HWC uint8, edges multiples of 64 (or 512 x 512 under --use_center_crop)
    valid_hw: tuple            # un-padded extent of net_in, () under --use_center_crop (nothing to remove)
    src: str = ""              # the input file (its caption under --caption_dir)
    # --resize gpu: lq is the DECODED file (nothing is resized on the host), net_in is None and valid_hw is geo.valid_hw
    geo: object = None         # resample.job_geometry() of the file: resize chain, valid extent, network size, LANCZOS target
    raw: np.ndarray = None     # the decoded file, HWC uint8: what is uploaded
    gt: np.ndarray = None      # --gt: the ground truth of a job that is scored on the device (png_rect() is not None), HWC uint8 of the saved size
    deg: object = None         # --degrade: the file's degrade.Params (raw is then ground truth; the device makes the LQ image)


def net_shape(job: Job) -> tuple:
    """Shape of the network input of a job, wherever it is made."""
    return job.net_in.shape if job.geo is None else tuple(job.geo.net_hw) + (3,)


def attach_gt(job: Job, args: Namespace) -> Job:
    """--gt: decode the ground truth of a job whose saved image is the device's image (png_rect), next to the input on the reader thread."""
    lookup = getattr(args, "gt_lookup", None)
    rect = png_rect(job, args) if lookup is not None else None
    if rect is not None:
        from instarevive_amd.metrics import MetricsError
        path = lookup.path(job.src)
        # --degrade without --gt: the decoded file is the ground truth (a file the device decodes has no pixels here: the scorer's copy is PIL's)
        same = job.deg is not None and os.path.abspath(path) == os.path.abspath(job.src) and isinstance(job.raw, np.ndarray)
        gt = job.raw if same else np.array(Image.open(path).convert("RGB"))
        if job.deg is not None and job.geo.crop is not None and gt.shape[:2] != tuple(rect):
            # --center_crop gpu under --degrade: what is degraded is the crop, so the ground truth is cropped as well - on the host, by the same rule
            from instarevive_amd.utils import center_crop_arr
            full = Image.fromarray(gt)
            if args.sr_scale != 1:
                full = full.resize(tuple(math.ceil(edge * args.sr_scale) for edge in full.size), Image.BICUBIC)
            gt = np.ascontiguousarray(center_crop_arr(full, rect[0]))
        if gt.shape[:2] != tuple(rect):
            raise MetricsError(f"--gt: {path} is {gt.shape[0]} x {gt.shape[1]}, the result of {job.src} is {rect[0]} x {rect[1]}")
        job.gt = gt
    return job


def read_job(file_path: str, repeat: int, args: Namespace) -> Job:
    return attach_gt(decode_job(file_path, repeat, args), args)


def decode_job(file_path: str, repeat: int, args: Namespace) -> Job:
    from instarevive_amd.utils import auto_resize, center_crop_arr, get_file_name_parts, pad
    source = device_source(file_path, args) if getattr(args, "resize_on_gpu", False) else None   # --jpeg_decoder gpu / --png_decoder gpu
    lq = Image.open(file_path).convert("RGB") if source is None else None
    if getattr(args, "resize_on_gpu", False):   # decode only: the sizes are worked out here, the pixels are resampled on the device
        from instarevive_amd.resample import crop_geometry, job_geometry
        width, height = lq.size if source is None else (source.shape[1], source.shape[0])
        if args.use_center_crop and crop_on_gpu(args):   # the device crops: the parameters of --degrade are drawn for the crop
            geo = crop_geometry((width, height), args.sr_scale, 512)
        else:
            geo = job_geometry((width, height), args.sr_scale, args.tiled, args.tile_size)
        folder, stem, _ = get_file_name_parts(os.path.join(args.output, os.path.relpath(file_path, args.input)))
        job = Job(os.path.join(folder, f"{stem}_{repeat}{save_ext(args)}"), lq, None, geo.valid_hw, file_path, geo, np.array(lq) if source is None else source)
        if getattr(args, "degrade_recipe", None):   # the draws (and the noise field) are made here, on a reader thread
            from instarevive_amd.degrade import draw
            job.deg = draw(args.degrade_recipe, os.path.relpath(file_path, args.input), *(geo.valid_hw if geo.crop is not None else (height, width)), args.degrade_seed)
        return job
    if args.sr_scale != 1:
        lq = lq.resize(tuple(math.ceil(edge * args.sr_scale) for edge in lq.size), Image.BICUBIC)
    if args.use_center_crop and not args.tiled:
        net_in = np.array(center_crop_arr(lq, 512))
    else:
        fitted = auto_resize(lq, args.tile_size if args.tiled else 512)
        net_in = pad(np.array(fitted), scale=64)
    # --use_center_crop switches the un-padding / resize-back of the result off, also next to --tiled (inference.py:326-346)
    valid = () if args.use_center_crop else (fitted.height, fitted.width)
    folder, stem, _ = get_file_name_parts(os.path.join(args.output, os.path.relpath(file_path, args.input)))
    return Job(os.path.join(folder, f"{stem}_{repeat}{save_ext(args)}"), lq, net_in, valid, file_path)


def png_rect(job: Job, args: Namespace):
    """The rectangle (vh, vw) of the prediction that write_job() would save unchanged, or None when the saved file is anything else. It is a plain
    crop when there is no --show_lq strip and the resize back to the LQ size is the identity: nothing to un-pad (--use_center_crop), or an LQ image
    that auto_resize left at its size (PIL's resize to the same size copies). Such jobs can be encoded on the GPU (--png_encoder gpu).
    A job that --resize gpu resizes on the device is saved as the device leaves it: the rectangle is its final size, the LANCZOS target of an
    enlarged input included."""
    if getattr(args, "show_lq", False):
        return None
    if job.geo is not None:
        return tuple(job.geo.lanczos[::-1]) if job.geo.lanczos else tuple(job.geo.valid_hw)
    if not job.valid_hw:
        return tuple(job.net_in.shape[:2])
    vh, vw = job.valid_hw
    return (vh, vw) if job.lq.size == (vw, vh) else None


def write_png_file(job: Job, blob) -> None:
    """write_job() for a result the GPU has encoded already: a PNG or JPEG file, or what process_stream(png_wrap=False) yields - the (zlib stream,
    width, height) triple of a PNG, the six pieces of a JPEG - framed here, on a writer thread, into one."""
    if not isinstance(blob, bytes) and len(blob) == 3:
        from instarevive_amd.png import wrap_png
        blob = wrap_png(*blob)
    elif not isinstance(blob, bytes):
        from instarevive_amd.jpeg import wrap_jpeg
        blob = wrap_jpeg(*blob)
    os.makedirs(os.path.dirname(job.save_path) or ".", exist_ok=True)
    with open(job.save_path, "wb") as f:
        f.write(blob)
    print(f"save to {job.save_path}")


def write_lq(job: Job, lq: np.ndarray, args: Namespace) -> None:
    """--save_lq: the LQ image the device synthesised, as DIR/<input-relative path>.png."""
    path = os.path.splitext(os.path.join(args.save_lq, os.path.relpath(job.src, args.input)))[0] + ".png"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(lq).save(path)
    print(f"save lq to {path}")


def write_job(job: Job, pred: np.ndarray, stage1_pred, args: Namespace) -> None:
    def back_to_lq(img):
        if not job.valid_hw or job.geo is not None:   # --resize gpu: the device has un-padded and resized it already
            return img
        img = img[:job.valid_hw[0], :job.valid_hw[1], :]
        return np.array(Image.fromarray(img).resize(job.lq.size, Image.LANCZOS))

    os.makedirs(os.path.dirname(job.save_path) or ".", exist_ok=True)
    result = back_to_lq(pred)
    if args.show_lq:
        panels = [np.array(job.lq) if job.valid_hw else job.net_in]
        if not args.disable_preprocess_model:
            panels.append(back_to_lq(stage1_pred))
        result = np.concatenate(panels + [result], axis=1)
    lvl = getattr(args, "png_compress_level", None)
    if getattr(args, "save_format", "png") == "jpg":   # the parameters that make PIL's file the device encoder's
        from instarevive_amd.jpeg import save_host, subsampling_of
        save_host(Image.fromarray(result), job.save_path, args.jpeg_quality, subsampling_of(args.jpeg_subsampling))
    elif lvl is None:
        Image.fromarray(result).save(job.save_path)
    else:
        Image.fromarray(result).save(job.save_path, compress_level=lvl)
    print(f"save to {job.save_path}")


class HostPools:
    """The host side of the stream (one main thread around an 8 images/s GPU delivers 0.6 - 1.2 files/s). Readers run
    read_job() ahead of the GPU, writers run write_job() behind it; both keep the reference's per-file arithmetic and file names
    (test_scripts/inference.py:263-291,323-346) - only WHEN a file is decoded or encoded changes, so the PNGs are pixel-identical to the
    one-thread run. Order is preserved on the read side (batches_of() groups CONSECUTIVE files, and the result list pairs with the job
    list by position); writes are independent files and may finish in any order. Both queues are bounded: at most `depth` decoded inputs
    wait for the GPU and at most `depth` results wait for an encoder, so memory stays at a few dozen images whatever the folder size.
    workers = 0 runs everything inline on the caller's thread (the reference's behaviour)."""

    def __init__(self, workers: int):
        self.workers = max(workers, 0)
        self.depth = max(2 * self.workers, 2)
        # reading (decode + bicubic + pad) is ~10x cheaper than writing (LANCZOS + PNG deflate): a quarter of the threads keeps up
        self.readers = ThreadPoolExecutor(max(1, self.workers // 4), thread_name_prefix="ir-read") if self.workers else None
        self.writers = ThreadPoolExecutor(self.workers, thread_name_prefix="ir-write") if self.workers else None
        self.slots = threading.Semaphore(self.depth)
        self.pending = deque()
        self.written = 0

    def read_ahead(self, fn: Callable, items: Iterable) -> Iterator:
        """fn(item) for every item, results in the items' order, up to `depth` calls running or finished ahead of the consumer."""
        if not self.readers:
            for item in items:
                yield fn(item)
            return
        ahead = deque()
        for item in items:
            ahead.append(self.readers.submit(fn, item))
            if len(ahead) >= self.depth:
                yield ahead.popleft().result()
        while ahead:
            yield ahead.popleft().result()

    def write_behind(self, fn: Callable, *a) -> None:
        """fn(*a) on a writer thread; blocks while `depth` writes are outstanding. A failed write is re-raised by the next call / drain()."""
        self.written += 1
        if not self.writers:
            fn(*a)
            return
        while self.pending and self.pending[0].done():
            self.pending.popleft().result()
        self.slots.acquire()

        def run():
            try:
                fn(*a)
            finally:
                self.slots.release()

        self.pending.append(self.writers.submit(run))

    def drain(self) -> None:
        while self.pending:
            self.pending.popleft().result()
        for pool in (self.readers, self.writers):
            if pool:
                pool.shutdown(wait=True)


def in_step(queue: deque) -> Iterator:
    """An endless iterator over what a batch generator appends to `queue` per batch it yields - the form process_stream(png= / resize= / gt= /
    niqe_rects= / degrade=) takes: it advances each right after it has drawn a batch."""
    while True:
        yield queue.popleft()


def batches_of(jobs: Iterable[Job], limit: int, key: Callable = None) -> Iterator[List[Job]]:
    """Consecutive jobs of equal network-input shape, at most `limit` per batch (limit 1 = the reference's one image per call). With `key`, jobs
    whose key(job) differs do not share a batch either (--png_encoder gpu: a batch is encoded on the GPU as a whole or not at all)."""
    group: List[Job] = []
    for job in jobs:
        if group and (len(group) >= limit or net_shape(job) != net_shape(group[0]) or (key is not None and key(job) != key(group[0]))):
            yield group
            group = []
        group.append(job)
    if group:
        yield group


def load_models(args: Namespace, device: torch.device) -> SimpleNamespace:
    from instarevive_amd.models import AutoencoderKL, DDPMScheduler, Transformer2DModel
    from instarevive_amd.utils import instantiate_from_config, load_state_dict, load_yaml
    m = SimpleNamespace()
    m.noise_scheduler = DDPMScheduler.from_pretrained(args.dit_config, subfolder="scheduler")
    m.vae = AutoencoderKL.from_pretrained(args.vae).to(torch.float32).to(device)
    m.model = Transformer2DModel.from_pretrained(args.dit_config, subfolder="transformer")
    m.model.load_state_dict(torch.load(args.ckpt, map_location="cpu"))
    m.preprocess_model = instantiate_from_config(load_yaml(args.swinir_config))
    load_state_dict(m.preprocess_model, torch.load(args.swinir_ckpt, map_location="cpu"), strict=True)
    m.model.to(device)
    m.preprocess_model.to(device)
    if getattr(args, "prompt", None) is not None:   # --prompt TEXT: text_prompts.setup() encodes the fixed prompt, no file is read
        m.y = m.y_mask = None
        return m
    prompt = torch.load(args.prompt_embeds, map_location="cpu")
    embeds = prompt["caption_embeds"]
    m.y = embeds.to(device, torch.float32).reshape(1, -1, embeds.shape[-1])
    # [1,1,L]: a 3-D mask reaches the cross-attention as an ADDITIVE bias (diffusers semantics, inference.py:274-277)
    m.y_mask = prompt["emb_mask"].to(device, torch.float32).reshape(1, 1, -1)
    return m


def main() -> None:
    from instarevive_amd import parallel
    from instarevive_amd.pipeline import HipTileEngine, process_stream
    from instarevive_amd.utils import list_image_files
    args = parse_args()
    check_text_prompts(args)
    check_save_format(args)
    check_center_crop(args)
    check_jpeg_decoder(args)
    check_png_decoder(args)
    topiq_model = load_topiq_model(args)
    niqe_params = load_niqe_params(args)
    ilniqe_params = load_ilniqe_params(args)
    if ilniqe_params is not None and args.shard_tiles:
        raise SystemExit("--ilniqe_params is not offered together with --shard_tiles (the assembled frame of the tile-sharded path is not scored on the device)")
    clipiqa_model = load_clipiqa_model(args)
    musiq_model = load_musiq_model(args)
    maniqa_model = load_maniqa_model(args)
    dists_weights = load_dists_weights(args)
    fid_weights, fid_stats = load_fid(args)
    noref = bool(niqe_params) or ilniqe_params is not None or clipiqa_model is not None or musiq_model is not None or maniqa_model is not None or topiq_model is not None
    if args.save_lq and not args.degrade:
        raise SystemExit("--save_lq writes the images --degrade synthesises: give --degrade as well")
    if args.degrade:
        from instarevive_amd import degrade as D
        try:
            D.check_flags(args)
            args.degrade_recipe = D.load_recipe(args.degrade)
        except (D.DegradeError, OSError, ValueError) as e:
            raise SystemExit(f"--degrade: {e}")
        if args.resize != "gpu":
            print(f"--degrade: the LQ images are made on the device, switching --resize gpu on")
            args.resize = "gpu"
        if not args.gt and (args.metrics_out or args.lpips_lin or noref or dists_weights or (fid_weights and fid_stats is None)):
            args.gt = args.input   # the files that are degraded are the ground truth of what is restored from them
    torch.manual_seed(args.seed)  # the path is deterministic; kept for surface compatibility (pl.seed_everything)
    args.device = check_device(args.device)
    rank, world, local = parallel.init_distributed()
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    m = load_models(args, device)
    from instarevive_amd import text_prompts
    text_caps = text_prompts.setup(args, m, device, log=lambda t: print(f"[rank {rank}] {t}"), max_batch=max(args.batch_size, 1))
    if args.fp8 != "off":
        from instarevive_amd import _lib as L
        if args.shard_tiles:
            raise SystemExit("--fp8 is not offered together with --shard_tiles (the sharded encode runs the bf16 attention)")
        m.vae.enable_fp8(True)                                   # packs + uploads the fp8 weight forms ...
        ctx = m.model.ctx
        ctx.check(ctx.lib.ir_set_fp8(ctx.h, 0), "ir_set_fp8")    # ... the mode itself is switched per call (IR_FLAG_FP8)
        if args.fp8 in ("default", "auto"):   # the operand set these weights allow (calibrated once per weight set, cached)
            from instarevive_amd import fp8_select
            fmask = fp8_select.auto_mask(m.preprocess_model, m.vae, m.model, m.y, m.y_mask, log=lambda t: print(f"[rank {rank}] {t}"))
            m.vae.enable_fp8(True)
            ctx.check(ctx.lib.ir_set_fp8(ctx.h, 0), "ir_set_fp8")
        else:
            fmask = {"qualified": L.FP8_MASK_QUALIFIED, "all": L.FP8_MASK_ALL, "attention": L.FP8_MASK_ATTENTION}[args.fp8]
        ctx.check(ctx.lib.ir_set_fp8_mask(ctx.h, fmask), "ir_set_fp8_mask")
        if fmask == 0:
            print(f"[rank {rank}] fp8: no operand part holds the tolerance on these weights - running bf16 throughout")
    report = None
    if (args.lpips_lin or args.lpips_alexnet) and not args.gt:
        raise SystemExit("--lpips_lin / --lpips_alexnet score against ground truth: give --gt as well")
    if args.lpips_alexnet and not args.lpips_lin:
        raise SystemExit("--lpips_alexnet needs --lpips_lin (the lpips linear heads)")
    if args.gt or noref:
        from instarevive_amd.metrics import GroundTruth, Report
        if args.shard_tiles:
            raise SystemExit("--gt / --niqe_params / --clipiqa_model / --musiq_model are not offered together with --shard_tiles, nor is --maniqa_model (the assembled frame of the tile-sharded path is not scored on the device)")
        if args.gt:
            args.gt_lookup = GroundTruth(args.gt, args.input)
        report = Report(args.metrics_out or os.path.join(args.output, "metrics.csv" if world == 1 else f"metrics.rank{rank}.csv"),
                        **({"lpips": True} if args.lpips_lin else {}), **({"niqe": True} if niqe_params else {}), **({"ilniqe": True} if ilniqe_params else {}), **({"clipiqa": True} if clipiqa_model else {}),
                        **({"musiq": True} if musiq_model else {}), **({"maniqa": True} if maniqa_model else {}), **({"paired": bool(args.gt)} if noref else {}),
                        **({"dists": True} if dists_weights else {}), **({"topiq_nr": True} if topiq_model else {}))
        if ilniqe_params:
            from instarevive_amd import ilniqe
            ilniqe.configure(m.model.ctx)
        if dists_weights:
            from instarevive_amd import dists
            dists.configure(m.model.ctx, dists_weights)
        if args.lpips_lin:
            from instarevive_amd import lpips
            lpips.configure(m.model.ctx, args.lpips_lin, args.lpips_alexnet)
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
    fid_run = None
    if fid_weights:
        from instarevive_amd import fid
        fid.configure(m.model.ctx, fid_weights)
        fid_run = fid.Run(fid.Run.default_path(args.output, args.fid_features_out), fid_stats, rank, world)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    if os.environ.get("IR_SWITCH_INTERVAL"):   # experiment knob: how long a worker thread may keep the GIL while the thread that feeds the GPU waits for it
        import sys
        sys.setswitchinterval(float(os.environ["IR_SWITCH_INTERVAL"]))
    pools = HostPools(default_workers(local_world) if args.workers < 0 else args.workers)
    gpu_png = args.png_encoder == "gpu"
    jpg = args.save_format == "jpg"
    gpu_jpg = jpg and args.jpeg_encoder == "gpu"
    on_gpu = gpu_png or gpu_jpg   # the files whose saved image is the device's image are coded there
    if jpg and report:
        print(f"[rank {rank}] --save_format jpg: the scores are those of the device's image, the result BEFORE the JPEG loss")
    args.resize_on_gpu = args.resize == "gpu"
    for flag, why in (("show_lq", "its strip needs the enlarged LQ panel on the host"), ("use_center_crop", "the centre crop halves with a BOX filter"),
                      ("shard_tiles", "the tile-sharded path takes host-prepared images")):
        if args.resize_on_gpu and getattr(args, flag) and not (flag == "use_center_crop" and crop_on_gpu(args)):
            print(f"[rank {rank}] --resize gpu: --{flag} keeps the resizes on the host ({why})")
            args.resize_on_gpu = False
    note = "" if jpg else host_keeps_up(pools.workers, int(512 * 512 * max(args.sr_scale, 1.0) ** 2), args.png_compress_level, args.png_encoder)   # priced on a 512 x 512 LQ file at this --sr_scale
    if note:
        print(f"[rank {rank}] {note}")
    if not os.path.isdir(args.input):
        raise SystemExit(f"--input {args.input} is not a directory")
    # os.walk order, like the reference (no sorting) for one process. With several ranks the list is what decides which rank owns
    # which file (and, under --shard_tiles, which image a collective belongs to), and os.walk promises no order across processes:
    # every rank sorts its listing and checks it against rank 0's.
    files = list_image_files(args.input, follow_links=True)
    if world > 1:
        files = parallel.agree_on_list(sorted(files))
    common = dict(color_fix_type=args.color_fix_type, disable_preprocess_model=args.disable_preprocess_model, tile_size=args.tile_size,
                  tile_stride=args.tile_stride, preprocess_model=m.preprocess_model, vae=m.vae, y=m.y, y_mask=m.y_mask,
                  noise_scheduler=m.noise_scheduler)
    caps = text_caps   # --captions: the same per-batch path as --caption_dir, with the prompts already on the device
    if args.caption_dir:
        from instarevive_amd.prompts import Captions
        caps = Captions(args.caption_dir, m.y, m.y_mask, args.input)
    host_files = 0   # --png_encoder gpu: files that were not a plain crop of the prediction and went through PIL
    if args.shard_tiles and args.tiled and world > 1:
        # one large image at a time, its tiles spread over the GPUs; rank 0 re-assembles and writes
        engine = HipTileEngine(m.model, m.vae, m.preprocess_model, m.y, m.y_mask, args.color_fix_type, args.disable_preprocess_model,
                               args.tile_size, args.tile_stride, m.noise_scheduler)
        for job in pools.read_ahead(lambda pi: read_job(pi[0], pi[1], args), [(p, i) for p in files for i in range(args.repeat_times)]):
            if caps:
                engine.y, engine.y_mask = caps.batch([job.src])
            rect = png_rect(job, args) if gpu_png else None
            preds, stage1 = parallel.sharded_tiled_process(engine, [job.net_in], rank, world, png=[rect] if rect else None, png_runs=args.png_runs)
            if rank == 0:
                host_files += rect is None
                if rect:   # rank 0 has encoded the assembled frame
                    pools.write_behind(write_png_file, job, preds[0])
                else:
                    pools.write_behind(write_job, job, preds[0], stage1[0], args)
        pools.drain()
        if text_caps:
            text_caps.finish()
        if gpu_png and rank == 0:
            print(f"[rank {rank}] --png_encoder gpu: {host_files} of {pools.written} files took the host encoder (not a plain crop of the prediction)")
        if gpu_jpg and rank == 0:
            print(f"[rank {rank}] --jpeg_encoder gpu: 0 of {pools.written} files were coded on the device (--shard_tiles keeps the host encoder, the same bytes)")
        return
    mine = parallel.shard(files, rank, world)       # images are independent: no collective on the data path
    t0 = time.perf_counter()
    jobs = pools.read_ahead(lambda pi: read_job(pi[0], pi[1], args), [(p, i) for p in mine for i in range(args.repeat_times)])
    todo: List[List[Job]] = []
    rects = deque()   # --png_encoder gpu, per batch drawn by process_stream: its rectangles, or None for a batch of the host encoder
    records = deque()   # --resize gpu, per batch: the decoded files and their geometry
    truths = deque()   # --gt, per batch: the ground-truth images, or None for a batch that is not scored
    names = deque()    # --maniqa_model, per batch: the saved files' names, which key random crops
    sizes = deque()    # --niqe_params / --clipiqa_model / --musiq_model / --maniqa_model, per batch: the saved sizes, or None for a batch that is not scored
    dparams = deque()  # --degrade, per batch: the files' degrade.Params
    fid_sizes = deque()   # --fid_model, per batch: the saved sizes, or None for a batch that does not enter the set
    lq_images = deque()   # --save_lq, per batch: the LQ images process_stream hands over right before the batch's results

    def feed():
        for group in batches_of(jobs, max(args.batch_size, 1), (lambda j: png_rect(j, args) is not None) if on_gpu or report or fid_run else None):
            todo.append(group)
            if args.gt:
                truths.append([j.gt for j in group] if all(j.gt is not None for j in group) else None)
            if noref:
                rr = [png_rect(j, args) for j in group]
                sizes.append(rr if all(rr) else None)
                if maniqa_model:
                    names.append([os.path.basename(j.save_path) for j in group])
            if on_gpu:
                rr = [png_rect(j, args) for j in group]
                rects.append(rr if all(rr) else None)
            if fid_run:   # with the ground truth as the reference set, a file enters only together with its ground truth
                rr = [png_rect(j, args) for j in group]
                fid_sizes.append(rr if all(rr) and (fid_stats is not None or all(j.gt is not None for j in group)) else None)
            imgs = [j.net_in for j in group]
            if args.resize_on_gpu:
                from instarevive_amd.resample import ResizeJob
                records.append([ResizeJob(j.raw, j.geo) for j in group])
                if args.degrade:
                    dparams.append([j.deg for j in group])
            yield (imgs, *caps.batch([j.src for j in group])) if caps else imgs

    first = None    # (time, files) when the first result left the GPU: what follows is the steady state (no library / workspace warm-up in it)
    unscored = 0    # --gt / --niqe_params / --clipiqa_model / --musiq_model / --maniqa_model: files whose saved image is not the device's image
    # files below 96 pixels on an edge or without two complete feature rows; files below 32 pixels on an edge; files of which a resized side rounds to 0
    no_score = {"niqe": 0, "ilniqe": 0, "clipiqa": 0, "musiq": 0, "maniqa": 0, "topiq_nr": 0, "dists": 0}   # topiq_nr: files with a side below 16; maniqa: files with a short side of 224 or less; dists: files below 16 x 16
    for out in process_stream(m.model, feed(), tiled=args.tiled, return_stage1=args.show_lq and not args.disable_preprocess_model,
                              fp8=args.fp8 != "off", png=in_step(rects) if gpu_png else None, png_wrap=False, png_runs=args.png_runs,
                              **({"jpeg": in_step(rects), "jpeg_quality": args.jpeg_quality, "jpeg_subsampling": args.jpeg_subsampling} if gpu_jpg else {}),
                              resize=in_step(records) if args.resize_on_gpu else None, gt=in_step(truths) if args.gt else None,
                              **({"lpips": True} if report and report.lpips else {}),
                              **({"niqe": niqe_params} if niqe_params else {}), **({"ilniqe": ilniqe_params} if ilniqe_params else {}),
                              **({"clipiqa": True} if clipiqa_model else {}),
                              **({"musiq": True} if musiq_model else {}), **({"maniqa": in_step(names)} if maniqa_model else {}),
                              **({"topiq": True} if topiq_model else {}),
                              **({"dists": True} if dists_weights else {}),
                              **({"fid": args.fid_resize, "fid_rects": in_step(fid_sizes)} if fid_run else {}),
                              **({"niqe_rects": in_step(sizes)} if noref else {}),
                              **({"degrade": in_step(dparams), "lq_sink": lq_images.append if args.save_lq else None} if args.degrade else {}), **common):
        preds, stage1 = out[:2]
        group = todo.pop(0)
        if fid_run:
            extra = out[-1] if isinstance(out[-1], dict) else None
            if extra is not None:
                out = out[:-1]
            fid_run.add([os.path.relpath(job.save_path, args.output) for job in group], extra)
        if args.save_lq:
            for job, lq in zip(group, lq_images.popleft()):
                pools.write_behind(write_lq, job, lq, args)
                pools.written -= 1   # a file counts once, by its result
        if report:
            if len(out) > 2:
                for job, score in zip(group, out[2][0]):
                    missing = report.unscored(score)   # NaN: the image has no NIQE, no CLIP-IQA, no MUSIQ or no MANIQA
                    if missing:
                        no_score[missing] += 1
                    else:
                        report.add_scores(os.path.relpath(job.save_path, args.output), score)
            else:
                unscored += len(group)
        last_result = time.perf_counter()
        if first is None:
            first = (last_result, len(group))
        for k, job in enumerate(group):
            if isinstance(preds[k], tuple):   # encoded on the GPU; the writer thread frames it
                pools.write_behind(write_png_file, job, preds[k])
            else:
                host_files += on_gpu
                pools.write_behind(write_job, job, preds[k], stage1[k] if stage1 else None, args)
    pools.drain()
    t1 = time.perf_counter()
    if text_caps:
        text_caps.finish()   # the device's status word: nothing outside the vocabulary or the cache reached it
        print(f"[rank {rank}] --captions: {text_caps.encoded} captions were T5-encoded in the run" + (f", {len(text_caps.saved)} caption files written to {args.save_captions}" if args.save_captions else ""))
    if jpeg_decoder_note(args):
        print(f"[rank {rank}] {jpeg_decoder_note(args)}")
    if png_decoder_note(args):
        print(f"[rank {rank}] {png_decoder_note(args)}")
    if gpu_png:
        print(f"[rank {rank}] --png_encoder gpu: {host_files} of {pools.written} files took the host encoder (not a plain crop of the prediction)")
    if gpu_jpg:
        print(f"[rank {rank}] --jpeg_encoder gpu: {pools.written - host_files} of {pools.written} files were coded on the device, {host_files} took the host "
              f"encoder (their saved image is not the device's image; the same bytes)")
    if report:
        lines = report.write()
        what = " / ".join(f for f, on in (("--gt", args.gt), ("--niqe_params", niqe_params), ("--ilniqe_params", ilniqe_params), ("--clipiqa_model", clipiqa_model), ("--musiq_model", musiq_model), ("--maniqa_model", maniqa_model), ("--topiq_model", topiq_model)) if on)
        print(f"[rank {rank}] {what}: scored {len(report.rows)} files" + (f" against {args.gt}" if args.gt else "") + f" -> {report.path}")
        for ln in lines:
            print(ln)
        if no_score["niqe"]:
            print(f"[rank {rank}] --niqe_params: {no_score['niqe']} of {pools.written} files were not scored (NIQE needs 96 x 96 blocks and two complete feature rows)")
        if no_score["ilniqe"]:
            print(f"[rank {rank}] --ilniqe_params: {no_score['ilniqe']} of {pools.written} files were not scored (IL-NIQE needs two complete feature rows)")
        if no_score["clipiqa"]:
            print(f"[rank {rank}] --clipiqa_model: {no_score['clipiqa']} of {pools.written} files were not scored (CLIP-IQA needs 32 x 32 pixels)")
        if no_score["musiq"]:
            print(f"[rank {rank}] --musiq_model: {no_score['musiq']} of {pools.written} files were not scored (a resized side rounds to 0)")
        if no_score["maniqa"]:
            print(f"[rank {rank}] --maniqa_model: {no_score['maniqa']} of {pools.written} files were not scored (MANIQA needs a short side above 224 pixels)")
        if no_score["topiq_nr"]:
            print(f"[rank {rank}] --topiq_model: {no_score['topiq_nr']} of {pools.written} files were not scored (TOPIQ-NR needs 16 x 16 pixels)")
        if no_score["dists"]:
            print(f"[rank {rank}] --dists_model: {no_score['dists']} of {pools.written} files were not scored (DISTS is scored from 16 x 16 pixels)")
        if unscored:
            print(f"[rank {rank}] {what}: {unscored} of {pools.written} files were not scored (their saved image is not the device's image: an input the host "
                  f"enlarged, or --show_lq) - use --resize gpu")
    if fid_run:
        fid_run.finish()
    if pools.written:
        # first read submitted -> last PNG closed, model loading excluded (bench.py --cli_files parses this line)
        rest, dt_rest = pools.written - first[1], t1 - first[0]
        print(f"[rank {rank}] wrote {pools.written} files in {t1 - t0:.3f} s = {pools.written / (t1 - t0):.3f} files/s ({pools.workers} host threads); "
              f"after the first result: {rest} files in {dt_rest:.3f} s = {rest / dt_rest:.3f} files/s"
              + (f"; results left the GPU at {rest / (last_result - first[0]):.3f} /s (the rest is the encoders' drain of the last files)" if rest and last_result > first[0] else ""))


if __name__ == "__main__":
    main()
