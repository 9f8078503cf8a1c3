"""Each producer -> consumer site of DESIGN.md section 20 alone, at the 512 x 512 pair's shapes: the producer kernel (attention, x2 resize,
deformable sampling, depth-wise convolution, grouped fc1) hands its result to its one consumer GEMM as fp32 or as pre-split planes
(ops.Planes), the planes only when the consumer's plan reads them, as the model decides.  Each pair is replayed from a HIP graph (20 pairs
per graph, 30 replays), the two forms alternating twice; median microseconds per pair.

  python tools/mb_producer_planes.py [out.json]        (profiles/presplit_producers_timing.json: "alone")"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from siu3r_amd import ops  # noqa: E402
from siu3r_amd.ops import ACT_GELU, ACT_RELU  # noqa: E402

dev = "cuda"
g = torch.Generator().manual_seed(0)
R = lambda *s: torch.randn(*s, generator=g).to(dev)
PAIRS, REPLAYS = 20, 30
WS = (torch.empty((ops.SPLITK_WS_FLOATS,), dtype=torch.float32, device=dev), torch.zeros((ops.SPLITK_COUNTERS,), dtype=torch.int32, device=dev))


def feeds(want, like, plan):
    """Planes over `like` when asked for and the consumer's plan reads them (as the model decides)"""
    if not want:
        return None
    with ops.splitk_scope(WS):
        pl = plan(like)
    if not pl.a_x3_ok:
        print(f"   (consumer {pl.kernel.decode()} cannot read planes: the site stays fp32)", flush=True)
        return None
    return ops.Planes(like, storage=like)


def timed(fn):
    """median / min / max us per call of fn, replayed from a graph"""
    with ops.splitk_scope(WS):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(gr, stream=s):
                for _ in range(PAIRS):
                    fn()
    ts = []
    for i in range(REPLAYS + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1) * 1e3 / PAIRS)
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def site(name, make):
    """make(planes: bool) -> (fn, kernel names) ; both forms interleaved twice"""
    res = {"fp32": [], "planes": []}
    kern = {}
    for rnd in range(2):
        for form in ("fp32", "planes"):
            fn = make(form == "planes")
            log = []
            ops.set_plan_log(log)
            with ops.splitk_scope(WS):
                fn()
            ops.set_plan_log(None)
            kern[form] = [pl.kernel.decode() for pl in log]
            res[form].append(timed(fn))
    out = dict(site=name, kernels=kern, rounds=res)
    f, p = min(r["median"] for r in res["fp32"]), min(r["median"] for r in res["planes"])
    out["fp32_us"], out["planes_us"], out["saved_us"] = f, p, f - p
    print(f"{name:12s} fp32 {[round(r['median'], 2) for r in res['fp32']]}  planes {[round(r['median'], 2) for r in res['planes']]}  saved {f - p:+.2f} us   consumer: {kern['planes'][-1]}", flush=True)
    return out


def lin(n, k, bias=True):
    return ops.pack_linear(R(n, k) / k ** 0.5, R(n) if bias else None, True)


def grouped(n, k):
    return ops.stack_packed([lin(n, k), lin(n, k)])


results = []

# ---- encoder: attention [2, 1025, 16 x 64] -> proj 2050 x 1024 x 1024 (+ residual, stats, planes out)
def enc(planes):
    Z, N, Cc, H = 2, 1025, 1024, 16
    qkv = R(Z, N, 3, H, 64)
    x, x1 = R(Z, N, Cc), torch.empty(Z, N, Cc, device=dev)
    s1, xp1, wp = ops.RowStats(x1), ops.Planes(x1), lin(Cc, Cc)
    a = torch.empty(Z, N, Cc, device=dev)
    ap = feeds(planes, a, lambda t: ops.linear(t, wp, residual=x, out=x1, stats_out=s1, planes_out=xp1, dry_run=True))
    att = dict(heads=H, head_dim=64, scale=0.125, split3=True)

    def fn():
        ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], out=a, planes_out=ap, planes_only=True, **att)
        ops.linear(a, wp, residual=x, out=x1, stats_out=s1, a_planes=ap, planes_out=xp1)
    return fn
results.append(site("enc_attn", enc))

# ---- decoder: attention [2, 1025, 12 x 64] -> grouped proj 2 x (1025 x 768 x 768)
def dec(planes):
    B, V, N, Cc, H = 1, 2, 1025, 768, 12
    qkv = R(B * V, N, 3, H, 64)
    x, x1 = R(B, V, N, Cc), torch.empty(B, V, N, Cc, device=dev)
    s1, wp = ops.RowStats(x1), grouped(Cc, Cc)
    a4 = torch.empty(B, V, N, Cc, device=dev)
    ap = feeds(planes, a4, lambda t: ops.linear_grouped(t, wp, residual=x, out=x1, stats_out=s1, dry_run=True))
    att = dict(heads=H, head_dim=64, scale=0.125, split3=True)

    def fn():
        ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], out=a4.view(B * V, N, Cc), planes_out=ap, planes_only=True, **att)
        ops.linear_grouped(a4, wp, residual=x, out=x1, stats_out=s1, a_planes=ap)
    return fn
results.append(site("dec_attn", dec))

# ---- decoder: grouped fc1 (GELU) 768 -> 3072 -> grouped fc2 3072 -> 768
def decfc(planes):
    B, V, N, Cc = 1, 2, 1025, 768
    x2, xo = R(B, V, N, Cc), torch.empty(B, V, N, Cc, device=dev)
    so, w1, w2 = ops.RowStats(xo), grouped(4 * Cc, Cc), grouped(Cc, 4 * Cc)
    h = torch.empty(B, V, N, 4 * Cc, device=dev)
    hp = feeds(planes, h, lambda t: ops.linear_grouped(t, w2, residual=x2, out=xo, stats_out=so, dry_run=True))

    def fn():
        ops.linear_grouped(x2, w1, act=ACT_GELU, out=h, planes_out=hp, planes_only=True)
        ops.linear_grouped(h, w2, residual=x2, out=xo, stats_out=so, a_planes=hp)
    return fn
results.append(site("dec_fc", decfc))

# ---- pts3d head: x2 resize -> 3 x 3 convolution (grouped heads: [1, 2, H, W, C])
def conv_site(hw, cin, cout, act):
    def make(planes):
        x = R(2, hw // 2, hw // 2, cin)
        w = ops.stack_packed([ops.pack_conv(R(cout, cin, 3, 3) / (3 * cin ** 0.5), R(cout), True) for _ in range(2)])
        up = torch.empty(1, 2, hw, hw, cin, device=dev)
        upp = feeds(planes, up, lambda t: ops.conv2d(t, w, pad=1, act=act, dry_run=True))

        def fn():
            ops.resize_bilinear(x, (hw, hw), True, out=up.view(2, hw, hw, cin), planes_out=upp, planes_only=True)
            ops.conv2d(up, w, pad=1, act=act, a_planes=upp)
        return fn
    return make
results.append(site("pts_resize", conv_site(512, 128, 128, ACT_RELU)))
results.append(site("pts_fusion", conv_site(256, 256, 128, 0)))

# ---- adapter extractor: sampling -> output_proj 10752 x 1024 x 1024; depth-wise convolution -> fc2 256 -> 1024
def msd(planes):
    B, h, w, heads, d = 2, 32, 32, 16, 64
    Q, Cc = 21 * (h * w // 4), heads * d
    value, c = R(B, h * w, Cc), R(B, Q, Cc)
    offs_aw = torch.cat((R(B, Q, heads * 4 * 2) * 2.0, R(B, Q, heads * 4)), 2).contiguous()
    ref = torch.rand(Q, 1, 2, generator=g).to(dev)
    wo = lin(Cc, Cc)
    samp = torch.empty(B, Q, Cc, device=dev)
    sp = feeds(planes, samp, lambda t: ops.linear(t, wo, residual=c, dry_run=True))

    def fn():
        ops.msdeform_sample(value, offs_aw, ref, [(h, w)], heads, 4, torch.float32, out=samp, planes_out=sp, planes_only=True)
        ops.linear(samp, wo, residual=c, a_planes=sp)
    return fn
results.append(site("ext_msd", msd))


def dw(planes):
    B, h, w, Cc = 2, 32, 32, 256
    N = 21 * (h * w // 4)
    f1, c = R(B, N, Cc), R(B, N, 1024)
    w9c, bias, w2 = R(9, Cc) / 3, R(Cc), lin(1024, Cc)
    f2 = torch.empty_like(f1)
    fp = feeds(planes, f2, lambda t: ops.linear(t, w2, residual=c, dry_run=True))

    def fn():
        ops.dwconv3x3_gelu(f1, w9c, bias, h, w, out=f2, planes_out=fp, planes_only=True)
        ops.linear(f2, w2, residual=c, a_planes=fp)
    return fn
results.append(site("ext_dw", dw))

json.dump(dict(board=torch.cuda.get_device_name(0), uuid=str(torch.cuda.get_device_properties(0).uuid) if hasattr(torch.cuda.get_device_properties(0), "uuid") else None,
               pairs_per_graph=PAIRS, replays=REPLAYS, sites=results), open(sys.argv[1] if len(sys.argv) > 1 else "producer_planes.json", "w"), indent=1)
