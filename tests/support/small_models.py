"""The three networks of process() at toy widths with seeded weights, on the GPU: for tests that need a whole path to run and do not care
what it computes (tests/test_models_gpu.py compares the same configurations with the oracle)."""
from oracle import dit as odit
from oracle import swinir as oswin
from oracle import vae as ovae
from tests.golden._det import det_input, det_state_dict

SWIN_SMALL = dict(embed_dim=60, depths=[2, 2], num_heads=[6, 6])
VAE_SMALL = dict(ch=32)
DIT_SMALL = dict(num_layers=2, num_attention_heads=4, attention_head_dim=72, sample_size=16, caption_channels=64)


def small_models():
    """(SwinIR, AutoencoderKL, Transformer2DModel) of instarevive_amd.models and a prompt y [1, 20, 64] on the GPU."""
    from instarevive_amd.models import AutoencoderKL, SwinIR, Transformer2DModel
    sw = dict(oswin.DEFAULT_CFG, **SWIN_SMALL)
    swin = SwinIR(img_size=64, patch_size=1, in_chans=3, embed_dim=sw["embed_dim"], depths=sw["depths"], num_heads=sw["num_heads"], window_size=8,
                  mlp_ratio=sw["mlp_ratio"], sf=8, img_range=1.0, upsampler="nearest+conv", resi_connection="1conv", unshuffle=True, unshuffle_scale=8)
    swin.load_state_dict(det_state_dict(oswin.state_dict_shapes(SWIN_SMALL), seed=101), strict=False)
    ch = VAE_SMALL["ch"]
    vae = AutoencoderKL(block_out_channels=(ch, 2 * ch, 4 * ch, 4 * ch))
    vae.load_state_dict(det_state_dict(ovae.state_dict_shapes(VAE_SMALL), seed=202), strict=True)
    d = dict(odit.DEFAULT_CFG, **DIT_SMALL)
    dit = Transformer2DModel(num_attention_heads=d["num_attention_heads"], attention_head_dim=d["attention_head_dim"], num_layers=d["num_layers"],
                             sample_size=d["sample_size"], caption_channels=d["caption_channels"],
                             cross_attention_dim=d["num_attention_heads"] * d["attention_head_dim"])
    dit.load_state_dict(det_state_dict(odit.state_dict_shapes(DIT_SMALL), seed=404), strict=True)
    y = det_input(9, (1, 20, DIT_SMALL["caption_channels"]), -1, 1)
    return swin.to("cuda"), vae.to("cuda"), dit.to("cuda"), y.cuda()
