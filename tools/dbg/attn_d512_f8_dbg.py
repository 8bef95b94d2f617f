"""Debug probe for flash_attn_d512_fp8_kernel: error by output d-tile, by query lane, and against references built from subsets of keys."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from instarevive_amd import Context
from instarevive_amd import _lib as L
from tests.support.fp8_tiles import decode_tiles_d512, quantise_q_d512, D512_TILE_BYTES

ctx = Context(0)
b, t, d = 1, int(sys.argv[1]) if len(sys.argv) > 1 else 1024, 512
g = torch.Generator(device="cuda").manual_seed(7)
q = torch.randn(b, t, d, generator=g, device="cuda").to(torch.bfloat16)
k = torch.randn(b, t, d, generator=g, device="cuda").to(torch.bfloat16)
v = torch.randn(b, t, d, generator=g, device="cuda").to(torch.bfloat16)
o = torch.empty(b, t, d, dtype=torch.int16, device="cuda")
ws = torch.zeros(b * (t // 64) * D512_TILE_BYTES + 4096 + (t + 64) * 512 * 2 + b * t * 512 * 2, dtype=torch.uint8, device="cuda")
scale = d ** -0.5
ctx.check(ctx.lib.ir_op_attention_d512_fp8(ctx.h, ctx.stream(), L.ptr(q.view(torch.int16)), L.ptr(k.view(torch.int16)), L.ptr(v.view(torch.int16)), L.ptr(o), b, t, scale, L.ptr(ws), ws.numel()), "x")
torch.cuda.synchronize()
Kd, Vd = decode_tiles_d512(ws, b, t)
got = o.view(torch.bfloat16)[0].float()
qd = quantise_q_d512(q[0], scale * 1.4426950408889634)
s2 = (qd.double() @ Kd[0].double().t()) * 0.6931471805599453
P = torch.softmax(s2, dim=-1)
ref = (P @ Vd[0].double()).float()
err = got - ref
print("overall rel-L2", float(err.norm() / ref.norm()), "got norm", float(got.norm()), "ref norm", float(ref.norm()))
print("by d-tile:", [round(float(err[:, 32 * i:32 * i + 32].norm() / ref[:, 32 * i:32 * i + 32].norm()), 3) for i in range(16)])
print("by query mod 32 (first 8):", [round(float(err[i::32].norm() / ref[i::32].norm()), 3) for i in range(8)])
print("by query block of 128 (first 8):", [round(float(err[128 * i:128 * i + 128].norm() / ref[128 * i:128 * i + 128].norm()), 3) for i in range(min(8, t // 128))])
# scale fit: got ~ a * ref ?
a = float((got * ref).sum() / (ref * ref).sum())
print("best scalar fit a =", a, "residual", float((got - a * ref).norm() / ref.norm()))
# subsets of key tiles
nt = t // 64
for name, mask in (("even tiles", torch.arange(t, device="cuda") // 64 % 2 == 0), ("odd tiles", torch.arange(t, device="cuda") // 64 % 2 == 1),
                   ("first tile only", torch.arange(t, device="cuda") < 64), ("all but last tile", torch.arange(t, device="cuda") < t - 64),
                   ("all but first", torch.arange(t, device="cuda") >= 64)):
    s3 = s2.clone(); s3[:, ~mask] = -1e30
    r3 = (torch.softmax(s3, dim=-1) @ Vd[0].double()).float()
    print(f"{name:20s} rel-L2 {float((got - r3).norm() / r3.norm()):.4f}")
# unnormalised comparison: numerator and denominator separately are not visible; check row sums ratio via projection
base = torch.arange(t, device="cuda") >= 64
res = []
for j in range(1, nt):
    mask = base & ~((torch.arange(t, device="cuda") // 64) == j)
    s3 = s2.clone(); s3[:, ~mask] = -1e30
    r3 = (torch.softmax(s3, dim=-1) @ Vd[0].double()).float()
    res.append(round(float((got - r3).norm() / r3.norm()), 3))
print("tile 0 excluded + tile j excluded:", res)
# least squares weights per tile: got * l_ref ~ sum_j w_j num_j  (per row); fit w_j over all rows and d
E = torch.exp(s2 - s2.max(dim=-1, keepdim=True).values)            # [t][t]
num = torch.stack([(E[:, 64 * j:64 * j + 64] @ Vd[0, 64 * j:64 * j + 64].double()) for j in range(nt)])   # [nt][t][512]
den = torch.stack([E[:, 64 * j:64 * j + 64].sum(-1) for j in range(nt)])                                   # [nt][t]
# model: got = sum_j w_j num_j / sum_j u_j den_j ; first assume u = w and solve linear: got * sum_j w_j den_j = sum_j w_j num_j -> sum_j w_j (num_j - got den_j) = 0 with w_1 = 1
A = (num - got.double()[None] * den[:, :, None]).reshape(nt, -1).t()     # [t*512][nt]
rhs = -A[:, 1]
cols = [j for j in range(nt) if j != 1]
w = torch.linalg.lstsq(A[:, cols], rhs[:, None]).solution[:, 0]
print("fitted per-tile weights (tile 1 = 1):", [round(float(x), 3) for x in w])
