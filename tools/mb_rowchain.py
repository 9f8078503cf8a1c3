"""The row chain that ends a pixel-decoder encoder layer (output_proj + residual, LayerNorm, fc1 + ReLU, fc2 + residual, LayerNorm; bf16x3)
at the network's shape, M = 10752 rows, H = 1024: the five launches against siu3r_rowchain_x3, graph-replayed back to back.
python tools/mb_rowchain.py [out.json]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from siu3r_amd import ops
from mb_gemm import graph_time

g = torch.Generator().manual_seed(0)
M, D, H = 10752, 256, 1024
r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
x, res = r(M, D), r(M, D)
wo, bo, w1, c1, w2, c2 = r(D, D) / 16, r(D), r(H, D) / 16, r(H), r(D, H) / 32, r(D)
g1, b1, g2, b2 = 1 + 0.5 * r(D), r(D), 1 + 0.5 * r(D), r(D)
po, p1, p2 = ops.pack_matrix(wo, bo, True), ops.pack_matrix(w1, c1, True), ops.pack_matrix(w2, c2, True)
pack = ops.pack_rowchain(wo, bo, g1, b1, w1, c1, w2, c2, g2, b2)
out = torch.empty_like(x)


def five():
    a = ops.linear(x, po, out_dtype=torch.float32, residual=res)
    z = ops.layernorm(a, g1, b1, 1e-5, torch.float32)
    h = ops.linear(z, p1, out_dtype=torch.float32, act=ops.ACT_RELU)
    o = ops.linear(h, p2, out_dtype=torch.float32, residual=z)
    return ops.layernorm(o, g2, b2, 1e-5, torch.float32)


def one():
    return ops.rowchain_x3(x, res, pack, H, 1e-5, 1e-5, out=out)


ref, got = five(), one()
err = ((got - ref).abs().amax(-1) / ref.abs().amax(-1)).max().item()
flop = 3 * 2.0 * M * D * (D + 2 * H)          # three bf16 MFMA passes per product
wbytes = (D * D + 2 * H * D) * 4              # hi + lo planes of the three matrices: what every workgroup streams
t5 = [graph_time(five, n=10) for _ in range(5)]
t1 = [graph_time(one, n=10) for _ in range(5)]
rec = dict(M=M, H=H, five_launches_us=[round(t * 1e6, 2) for t in t5], rowchain_us=[round(t * 1e6, 2) for t in t1],
           five_tflops=round(flop / min(t5) / 1e12, 1), rowchain_tflops=round(flop / min(t1) / 1e12, 1),
           workgroups=(M + 63) // 64, weight_bytes_per_workgroup=wbytes, weight_gbps_per_cu=round(wbytes / min(t1) / 1e9, 1),
           max_row_difference=err, bit_identical=bool(torch.equal(got, ref)))
print(f"five launches {min(t5) * 1e6:7.1f} us ({rec['five_tflops']} TFLOP/s of bf16 MFMA issue)   siu3r_rowchain_x3 {min(t1) * 1e6:7.1f} us "
      f"({rec['rowchain_tflops']} TFLOP/s; {wbytes / 1e6:.2f} MB of weights per workgroup = {rec['weight_gbps_per_cu']} GB/s per CU)   max row difference {err:.2e} (bit-identical: {rec['bit_identical']})")
print(json.dumps(rec))
if len(sys.argv) > 1:
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
