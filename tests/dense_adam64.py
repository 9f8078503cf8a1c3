"""Dense restatement of the fused Adam step (siu3r_amd/optim.py::GaussianAdam, csrc/gaussian_adam.hip) in plain torch, parametrised by
dtype.  float64 is the reference of the GPU tests, float32 the 'composed torch update' their tolerance is taken from.

One field is (param, grad, exp_avg, exp_avg_sq), all [G, ...]; a row g is visible iff visible[g].  A visible row, in `dtype` and in this order:
  m = b1 m + (1 - b1) g;  v = b2 v + ((1 - b2) g) g;  p = p - ((lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps)
with 1 - b1, 1 - b2, bc1 = 1 - b1^t, bc2 = 1 - b2^t computed in Python doubles and then converted, as the host side of the kernel does.  The element with
index i within its row (flattened) steps with lr when head_period == 0 or i % head_period == 0, and with lr_tail otherwise.  An invisible
row keeps param, exp_avg and exp_avg_sq and its grad is not looked at (torch.where on the inputs: a NaN there does not reach the output)."""
import torch

FIELD_WIDTHS = lambda n: {"means": (3,), "scales": (3,), "rotations": (4,), "opacities": (), "harmonics": (3, n)}
LRS = {"means": 1.6e-4, "scales": 5e-3, "rotations": 1e-3, "opacities": 5e-2, "harmonics": 2.5e-3}


def visible_rows(visible, G):
    """bool [G] from None (all), int32 radii [V,G,R] (any entry > 0) or a bool / uint8 mask [G]"""
    if visible is None:
        return torch.ones(G, dtype=torch.bool)
    if visible.dtype == torch.int32:
        return (visible > 0).any(-1).any(0)
    return visible.bool()


def step(p, g, m, v, t, lr, lr_tail=None, head_period=0, betas=(0.9, 0.999), eps=1e-15, visible=None, dtype=torch.float64):
    """one step of one field -> (p, m, v) new tensors of `dtype`; the inputs are converted (an upcast of float32 is exact) and not modified"""
    G = p.shape[0]
    c = lambda x: x.detach().to(dtype)
    s = lambda x: torch.tensor(float(x), dtype=dtype)
    p0, g0, m0, v0 = c(p), c(g), c(m), c(v)
    b1, b2 = s(betas[0]), s(betas[1])
    bc1, bc2 = s(1.0 - float(betas[0]) ** t), s(1.0 - float(betas[1]) ** t)
    width = p0[0].numel()
    idx = torch.arange(width)
    head = torch.ones(width, dtype=torch.bool) if head_period == 0 else idx % head_period == 0
    lr_e = torch.where(head, s(lr), s(lr if lr_tail is None else lr_tail)).reshape(p0.shape[1:])
    vis = visible_rows(visible, G).reshape((G,) + (1,) * (p0.dim() - 1))
    gs = torch.where(vis, g0, torch.zeros_like(g0))  # (an invisible row's gradient is never read)
    m1 = b1 * m0 + s(1.0 - float(betas[0])) * gs
    v1 = b2 * v0 + s(1.0 - float(betas[1])) * gs * gs
    p1 = p0 - (lr_e / bc1) * m1 / (torch.sqrt(v1) / torch.sqrt(bc2) + s(eps))
    return torch.where(vis, p1, p0), torch.where(vis, m1, m0), torch.where(vis, v1, v0)


def make_field(kind, shape, seed, state="fresh"):
    """Seeded float32 (param, grad, exp_avg, exp_avg_sq, t) on the CPU.  Gradients have a per-row scale spread log-uniformly over 1e-8 .. 1 and
    one row in seven exactly zero.  "noise": parameters and gradients independent normals; "render": what a render's backward leaves: the
    gradient of neighbouring rows shares its sign pattern and 30 % of the elements of a non-zero row are exactly zero too.  state "fresh":
    m = v = 0, t = 1; "t2" / "t1000": a running state with exp_avg ~ the gradient's scale and exp_avg_sq >= 0, t = 2 / 1000."""
    G = shape[0]
    gen = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(shape, generator=gen)
    row = lambda x: x.reshape((G,) + (1,) * (len(shape) - 1))
    scale = row(10.0 ** (-8.0 * torch.rand(G, generator=gen)))
    p = rn() * 2.0
    if kind == "noise":
        g = rn() * scale
    elif kind == "render":
        base = torch.randn(shape[1:], generator=gen)
        g = (base + 0.3 * rn()) * scale
        g[torch.rand(shape, generator=gen) < 0.3] = 0.0
    else:
        raise ValueError(kind)
    g[torch.arange(G) % 7 == 3] = 0.0
    if state == "fresh":
        m, v, t = torch.zeros(shape), torch.zeros(shape), 1
    elif state in ("t2", "t1000"):
        t = int(state[1:])
        m = 0.5 * rn() * scale
        v = (0.1 + torch.rand(shape, generator=gen)) * scale * scale
        v[torch.arange(G) % 11 == 5] = 0.0
        assert bool((v >= 0).all())
    else:
        raise ValueError(state)
    return p.float().contiguous(), g.float().contiguous(), m.float().contiguous(), v.float().contiguous(), t


def make_radii(G, V, seed, share=0.5, R=2):
    """int32 radii [V,G,R] under which about `share` of the rows are visible: an invisible row holds 0 and negative entries only, a visible
    row a positive entry in at least one view (often only one, and only one of its R entries)"""
    gen = torch.Generator().manual_seed(seed)
    vis = torch.rand(G, generator=gen) < share
    radii = -torch.randint(0, 3, (V, G, R), generator=gen, dtype=torch.int32)
    view = torch.randint(0, V, (G,), generator=gen)
    slot = torch.randint(0, R, (G,), generator=gen)
    rows = torch.nonzero(vis).flatten()
    radii[view[rows], rows, slot[rows]] = torch.randint(1, 40, (len(rows),), generator=gen, dtype=torch.int32)
    also = rows[torch.rand(len(rows), generator=gen) < 0.5]
    radii[(view[also] + 1) % V, also, :] = 7
    assert torch.equal(visible_rows(radii, G), vis)
    return radii.contiguous(), vis
