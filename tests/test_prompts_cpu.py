"""Per-image captions on the host (instarevive_amd.prompts: the reference's caption files, lookup rules, batch layout, the fixed-prompt fallback,
the equal-length rule), the per-row key bias of set_prompt, and the argument refusals of the new C-ABI entry points that need no device."""
import numpy as np
import pytest
import torch

from instarevive_amd import prompts as PR
from instarevive_amd.models import prompt_bias


def _save(path, ntok=6, dim=8, seed=0, mask=True):
    g = np.random.default_rng(seed)
    y = g.standard_normal((1, ntok, dim)).astype(np.float32)
    m = (np.arange(ntok) < ntok - 2).astype(np.float32)[None]
    path.parent.mkdir(parents=True, exist_ok=True)
    if mask:
        np.savez(path, caption_feature=y, attention_mask=m)
    else:
        np.savez(path, caption_feature=y)
    return y[0], m[0]


def _fallback(ntok=6, dim=8):
    return torch.full((1, ntok, dim), 0.5), torch.ones(1, 1, ntok) * torch.tensor([1, 1, 1, 0, 0, 0.0])


def test_load_caption_reads_the_reference_format(tmp_path):
    y, m = _save(tmp_path / "a.npz", seed=1)
    gy, gm = PR.load_caption(str(tmp_path / "a.npz"))
    assert gy.dtype == torch.float32 and gy.shape == (6, 8) and np.array_equal(gy.numpy(), y)
    assert np.array_equal(gm.numpy(), m)
    _save(tmp_path / "b.npz", seed=2, mask=False)   # no attention_mask: every token is real
    assert torch.equal(PR.load_caption(str(tmp_path / "b.npz"))[1], torch.ones(6))
    np.savez(tmp_path / "c.npz", other=np.zeros(3))
    with pytest.raises(PR.CaptionError, match="caption_feature"):
        PR.load_caption(str(tmp_path / "c.npz"))
    (tmp_path / "d.npz").write_bytes(b"not a zip")
    with pytest.raises(PR.CaptionError, match="d.npz"):
        PR.load_caption(str(tmp_path / "d.npz"))


def test_lookup_relative_path_first_then_flat_stem(tmp_path):
    caps, inp = tmp_path / "caps", tmp_path / "in"
    _save(caps / "sub" / "x.npz", seed=3)
    _save(caps / "x.npz", seed=4)
    _save(caps / "y.npz", seed=5)
    assert PR.caption_file(str(caps), str(inp / "sub" / "x.png"), str(inp)) == str(caps / "sub" / "x.npz")   # input-relative layout wins
    assert PR.caption_file(str(caps), str(inp / "x.jpg"), str(inp)) == str(caps / "x.npz")
    assert PR.caption_file(str(caps), str(inp / "deep" / "y.png"), str(inp)) == str(caps / "y.npz")        # the reference's flat layout
    assert PR.caption_file(str(caps), str(inp / "z.png"), str(inp)) is None


def test_batch_layout_and_fallback(tmp_path):
    caps, inp = tmp_path / "caps", tmp_path / "in"
    ya, ma = _save(caps / "a.npz", seed=6)
    yc, _ = _save(caps / "c.npz", seed=7, mask=False)
    fy, fm = _fallback()
    c = PR.Captions(str(caps), fy, fm, str(inp))
    y, m = c.batch([str(inp / "a.png"), str(inp / "b.png"), str(inp / "c.png")])
    assert y.shape == (3, 6, 8) and m.shape == (3, 1, 6)   # [B, T, 4096] / [B, 1, T]: the reference CLI's 3-D mask form
    assert np.array_equal(y[0].numpy(), ya) and np.array_equal(m[0, 0].numpy(), ma)
    assert torch.equal(y[1], fy[0]) and torch.equal(m[1, 0], fm.reshape(-1))   # no caption file: the --prompt_embeds prompt
    assert np.array_equal(y[2].numpy(), yc) and torch.equal(m[2, 0], torch.ones(6))


def test_unequal_token_counts_are_refused_with_the_file(tmp_path):
    caps = tmp_path / "caps"
    _save(caps / "long.npz", ntok=9, seed=8)
    fy, fm = _fallback()
    c = PR.Captions(str(caps), fy, fm)
    with pytest.raises(PR.CaptionError, match="long.npz"):
        c.batch([str(tmp_path / "long.png")])


def test_prompt_bias_per_row():
    m2 = torch.tensor([[1.0, 1, 0], [1, 0, 0]])
    assert torch.equal(prompt_bias(m2, 2, 3), (1 - m2) * -10000.0)             # 2-D: (1 - m) * -10000, row by row
    m3 = m2[:, None, :]
    assert torch.equal(prompt_bias(m3, 2, 3), m2)                              # 3-D: the additive bias as is
    assert torch.equal(prompt_bias(m3[:1], 2, 3), m2[:1].expand(2, -1))        # one mask row serves every prompt row
    assert torch.equal(prompt_bias(None, 2, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError):
        prompt_bias(m3, 3, 3)                                                  # two different rows for three prompts


def test_c_abi_refusals_without_a_device():
    from instarevive_amd import _lib
    from instarevive_amd.build import build
    build()
    lib = _lib.load_library()
    assert lib.ir_dit_set_prompts(None, None, None, None, 2, 10) == -1
    assert lib.ir_graph_records(None) == 0
    assert lib.ir_workspace_bytes(None, _lib.STAGE_DIT, 2, 64, 64, 0, 0, 0) == 0
    args = (None, None, None, None, None, None)
    assert lib.ir_op_attention_kv_groups(*args, 3, 2, 64, 20, 72, 0.1, None, 2, None, 0) == -2    # 3 items, 2 groups
    assert lib.ir_op_attention_kv_groups(*args, 4, 2, 64, 20, 72, 0.1, None, 0, None, 0) == -2    # no groups
    assert lib.ir_op_attention_kv_groups(*args, 4, 1, 64, 64, 512, 0.1, None, 2, None, 0) == -5   # no d = 512 form
    assert lib.ir_op_attention_kv_groups(*args, 4, 2, 64, 20, 72, 0.1, None, 2, None, 1024) == -20   # workspace for 2 K / V sets
