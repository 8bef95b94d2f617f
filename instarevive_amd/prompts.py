"""Per-image captions on the host: the reference's caption files (dataset/codeformer.py:765-790: `<caption_dir>/<image stem>.npz` holding
`caption_feature` [1, T, 4096] and an optional `attention_mask`) and the batches the DiT takes from them (y [B, T, 4096], y_mask [B, 1, T], the 3-D
form in which test_scripts/inference.py:273-277 passes its fixed prompt's mask, used as an additive bias as is).

An image without a caption file gets the fixed prompt (--prompt_embeds). All prompts of a run must have the same token count T: a padded prompt
would change results, because the reference's 3-D mask is added to the scores rather than masking the padding out.
"""
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch


class CaptionError(ValueError):
    pass


def caption_file(caption_dir: str, image_path: str, input_root: Optional[str] = None) -> Optional[str]:
    """The caption file of an image, or None: `caption_dir/<path relative to input_root, without extension>.npz` first, then
    `caption_dir/<file stem>.npz` (the reference's flat layout)."""
    stem = os.path.splitext(os.path.basename(image_path))[0]
    cands = []
    if input_root is not None:
        rel = os.path.relpath(image_path, input_root)
        if not rel.startswith(".."):
            cands.append(os.path.join(caption_dir, os.path.splitext(rel)[0] + ".npz"))
    cands.append(os.path.join(caption_dir, stem + ".npz"))
    for c in cands:
        if os.path.isfile(c):
            return c
    return None


def load_caption(path: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """One caption file -> (y [T, 4096] fp32, mask [T] fp32). A missing attention_mask means every token is real (all ones)."""
    try:
        with np.load(path) as d:
            if "caption_feature" not in d:
                raise CaptionError(f"{path}: no 'caption_feature' array")
            y = np.asarray(d["caption_feature"], dtype=np.float32)
            m = np.asarray(d["attention_mask"], dtype=np.float32) if "attention_mask" in d else None
    except CaptionError:
        raise
    except Exception as e:   # (a damaged archive raises zipfile / pickle errors as well as OSError / ValueError)
        raise CaptionError(f"{path}: not a caption file ({e})") from e
    if y.ndim == 3 and y.shape[0] == 1:
        y = y[0]
    if y.ndim != 2:
        raise CaptionError(f"{path}: caption_feature must be [1, T, C] or [T, C], got {list(y.shape)}")
    if m is None:
        m = np.ones(y.shape[0], dtype=np.float32)
    m = m.reshape(-1)
    if m.shape[0] != y.shape[0]:
        raise CaptionError(f"{path}: attention_mask has {m.shape[0]} entries for {y.shape[0]} tokens")
    return torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(np.ascontiguousarray(m))


class Captions:
    """The prompts of a run: per-image caption files under `caption_dir`, the fixed prompt (y [.., T, C], y_mask [.., T]) for images without one."""

    def __init__(self, caption_dir: str, fallback_y: torch.Tensor, fallback_mask: torch.Tensor, input_root: Optional[str] = None):
        self.caption_dir, self.input_root = caption_dir, input_root
        self.fb_y = fallback_y.detach().to("cpu", torch.float32).reshape(-1, fallback_y.shape[-2], fallback_y.shape[-1])[0].contiguous()
        self.fb_m = fallback_mask.detach().to("cpu", torch.float32).reshape(-1, fallback_mask.shape[-1])[0].contiguous()
        self.n_tok, self.dim = self.fb_y.shape
        if self.fb_m.shape[0] != self.n_tok:
            raise CaptionError(f"the fixed prompt's mask has {self.fb_m.shape[0]} entries for {self.n_tok} tokens")

    def prompt(self, image_path: str) -> Tuple[torch.Tensor, torch.Tensor, Optional[str]]:
        """(y [T, C], mask [T], caption file or None) of one image."""
        path = caption_file(self.caption_dir, image_path, self.input_root)
        if path is None:
            return self.fb_y, self.fb_m, None
        y, m = load_caption(path)
        if y.shape != (self.n_tok, self.dim):
            raise CaptionError(f"{path}: caption_feature is {list(y.shape)}, the run's prompts are [{self.n_tok}, {self.dim}] "
                               f"(every prompt of a run needs the same token count: padding would change results)")
        return y, m, path

    def batch(self, image_paths: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        """(y [B, T, C], y_mask [B, 1, T]) of a batch of images, in order."""
        ys, ms = zip(*[self.prompt(p)[:2] for p in image_paths])
        return torch.stack(ys), torch.stack(ms)[:, None, :]
