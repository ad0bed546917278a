"""include/mi3d.h Part 18 restated: the shading pass of a mesh with a float texture, its adjoint in the colour source with
the header's 64-bit fixed-point sums (NumPy, the bytes the GPU tests compare with), and the same pass in torch float64
under autograd - the truth the other two are measured against.  Built on mesh_render_model: the winners `tri` and the
perspective-correct weights `bary` are Part 17's and are taken from its shade().

A PLAN (plan()) lists, for every drawn pixel, the K elements of the colour source it reads and their weights: K = 3
vertices with w_k = lambda_k, or K = 4 texels (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1) with hx hy, fx hy,
hx fy, fx fy.  image[p] = sum_k w_k source[a_k]: the pass is linear, so its adjoint is grad[a] = sum over (p, k) with
a_k(p) = a of w_k g[p].

THE BOUND of the binary32 fixed-point gradient against exact arithmetic (bound(); u = 2^-24), by the method of Part 15's
"ERROR AGAINST EXACT ARITHMETIC" - first-order running bounds counted from the rounding chain:
  - a vertex weight carries Part 17's E(lambda_k) (mesh_render_model's Ebary);
  - a texel coordinate gx = u T - 0.5 carries E(gx) = T E(u) + u (|u T| + |gx|), gy = (1 - v) T - 0.5 carries
    E(gy) = T (E(v) + u |1 - v|) + u (|(1 - v) T| + |gy|); the four tap weights are the products of two hat functions of
    slope 1 and height 1 in gx and gy, evaluated with 2 roundings per factor (the subtraction g - i0 and 1 - f) and one
    for the product: every tap weight moves by at most E(gx) + E(gy) + 5 u - also when floor() falls on the other side
    in the two precisions, because the hat is continuous: the weight then moves from one texel's list to its
    neighbour's, and the bound is charged to the taps of BOTH plans;
  - TWO ROUNDINGS PER CONTRIBUTION: t = w g rounds once, u |w g|; llrint rounds once more, 2^(e - 1); so a sum of n
    contributions is off by at most sum (|g| E(w) + u |w g|) + n 2^(e - 1);
  - the result is rounded to binary64 and then to binary32: (u + 2^-53) |grad|, counted as 2 u |grad|.

Not a test module: helpers only."""
import numpy as np

import mesh_render_model as R

U = R.U
F = np.float32
QUIET_NAN = np.uint32(0x7FC00000)


# ------------------------------------------------------------------------------------------------ the plan

def plan(vertices, triangles, records, H, W, tri, vt=None, T=None, dtype=np.float32, bounds=False):
    """For the winners tri int64 [V, H, W] (-1: nothing drawn): a dict of `pixel` int64 [n] (flat index into V H W),
    `index` int64 [n, K] (the element of the source, without the channel), `weight` [n, K] of `dtype`; with a texture
    also i0, j0, fx, fy.  With bounds (dtype = np.float64) also `Eweight` [n, K] or, textured, [n]: the header's bounds."""
    out = R.shade(vertices, triangles, records, H, W, tri, colors=np.zeros((len(vertices), 3), F), F=dtype, bounds=bounds)
    if bounds and vt is not None:                                # Euv needs the texture path of shade()
        out = R.shade(vertices, triangles, records, H, W, tri, vt=vt, texture=np.zeros((T, T, 3), np.uint8), F=dtype,
                      bounds=True)
    drawn = tri.reshape(-1) >= 0
    pixel = np.flatnonzero(drawn)
    t = tri.reshape(-1)[pixel]
    lam = out["bary"].reshape(-1, 3)[pixel]
    p = dict(pixel=pixel)
    if vt is None:
        p["index"], p["weight"] = np.asarray(triangles)[t].astype(np.int64), lam
        if bounds:
            p["Eweight"] = out["Ebary"].reshape(-1, 3)[pixel]
        return p
    D = dtype
    uv = np.asarray(vt, F).astype(D).reshape(-1, 3, 2)[t]
    l3 = [lam[:, k] for k in range(3)]
    u, v = R._mix(l3, [uv[:, k, 0] for k in range(3)]), R._mix(l3, [uv[:, k, 1] for k in range(3)])
    gx, gy = u * D(T) - D(0.5), (D(1.0) - v) * D(T) - D(0.5)
    (i0, fx), (j0, fy) = R._tap(gx, T, D), R._tap(gy, T, D)
    hx, hy = D(1.0) - fx, D(1.0) - fy
    at = j0 * T + i0
    p.update(i0=i0, j0=j0, fx=fx, fy=fy, index=np.stack([at, at + 1, at + T, at + T + 1], -1),
             weight=np.stack([hx * hy, fx * hy, hx * fy, fx * fy], -1))
    if bounds:
        Euv = out["Euv"].reshape(-1, 2)[pixel]
        Egx = T * Euv[:, 0] + U * (abs(u * T) + abs(gx))
        Egy = T * (Euv[:, 1] + U * abs(1.0 - v)) + U * (abs((1.0 - v) * T) + abs(gy))
        p["Eweight"] = Egx + Egy + 5 * U
    return p


# ------------------------------------------------------------------------------------------------ the f32 forward

def shade_f32(p, texture, shape, background):
    """mi3d_mesh_shade_f32's image [V, H, W, 3] from a textured binary32 plan: top = c00 hx + c10 fx, bot = c01 hx + c11 fx,
    c = top hy + bot fy, every operation rounded separately, no / 255; the background elsewhere."""
    tex = np.asarray(texture, F)
    image = np.empty(tuple(shape) + (3,), F)
    image[:] = np.asarray(background, F)
    i0, j0, fx, fy = p["i0"], p["j0"], p["fx"][:, None], p["fy"][:, None]
    hx, hy = F(1.0) - fx, F(1.0) - fy
    top = tex[j0, i0] * hx + tex[j0, i0 + 1] * fx
    bot = tex[j0 + 1, i0] * hx + tex[j0 + 1, i0 + 1] * fx
    image.reshape(-1, 3)[p["pixel"]] = top * hy + bot * fy
    return image


# ------------------------------------------------------------------------------------------------ the backward

def amax_bits(dimage):
    """Launch 1: the largest bits(|g|) as a uint32; a NaN's bits exceed infinity's."""
    bits = np.ascontiguousarray(dimage, F).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return int(bits.max()) if bits.size else 0


def levels(N):
    """L: the smallest integer with 2^L >= N."""
    L = 0
    while (1 << L) < N:
        L += 1
    return L


def exponent(bits, N):
    """e = (E + 1) + L - 60 with E = (bits >> 23) - 127: 2^(E + 1) > amax, denormals included."""
    return ((bits >> 23) - 127 + 1) + levels(N) - 60


def contributions(w, g, e, L):
    """llrint(ldexp((double)(w * g), -e)), saturated at +-2^(61 - L), 0 for a NaN: int64; w and g binary32."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = (np.asarray(w, F) * np.asarray(g, F)).astype(F)
        x = np.ldexp(t.astype(np.float64), -e)
    cap = np.ldexp(1.0, 61 - L)
    x = np.where(np.isnan(x), 0.0, np.clip(x, -cap, cap))
    return np.rint(x).astype(np.int64)                          # to nearest, ties to even


def backward(p, dimage, elements, return_sums=False):
    """mi3d_mesh_shade_backward from a binary32 plan: dimage [V, H, W, 3] -> the gradient float32 [elements, 3]."""
    g = np.ascontiguousarray(dimage, F).reshape(-1, 3)
    N = len(g)
    bits = amax_bits(g)
    acc = np.zeros(elements * 3, np.int64)
    if bits >= 0x7F800000:
        grad = np.full(elements * 3, QUIET_NAN, np.uint32).view(F)
        return (grad.reshape(elements, 3), acc, None) if return_sums else grad.reshape(elements, 3)
    if bits == 0:
        grad = np.zeros((elements, 3), F)
        return (grad, acc, None) if return_sums else grad
    e, L = exponent(bits, N), levels(N)
    gp = g[p["pixel"]]
    for k in range(p["index"].shape[1]):
        for c in range(3):
            np.add.at(acc, p["index"][:, k] * 3 + c, contributions(p["weight"][:, k], gp[:, c], e, L))
    with np.errstate(over="ignore", under="ignore"):
        grad = np.ldexp(acc.astype(np.float64), e).astype(F).reshape(elements, 3)
    return (grad, acc, e) if return_sums else grad


def bound(p64, p32, dimage, elements, grad):
    """The header's bound on |binary32 fixed-point gradient - exact gradient| per entry [elements, 3]: p64 the binary64
    plan with bounds, p32 the binary32 plan (for the taps binary32 chose), grad the binary32 result."""
    g = np.abs(np.ascontiguousarray(dimage, np.float64).reshape(-1, 3))
    e = exponent(amax_bits(dimage), len(g))
    out = np.zeros((elements, 3))
    count = np.zeros(elements)
    gp = g[p64["pixel"]]
    K = p64["index"].shape[1]
    for k in range(K):
        Ew = p64["Eweight"][:, k] if p64["Eweight"].ndim == 2 else p64["Eweight"]
        for plan_ in ((p64, p32) if K == 4 else (p64,)):
            np.add.at(out, plan_["index"][:, k], (Ew + U * np.abs(p64["weight"][:, k]))[:, None] * gp)
        np.add.at(count, p32["index"][:, k], 1)
    return out + (count * 2.0 ** (e - 1))[:, None] + 2 * U * np.abs(grad.astype(np.float64))


# ------------------------------------------------------------------------------------------------ torch float64: the truth

def torch_plan(p, dtype, device="cpu"):
    import torch
    return dict(pixel=torch.from_numpy(p["pixel"]).to(device), index=torch.from_numpy(p["index"]).to(device),
                weight=torch.from_numpy(np.ascontiguousarray(p["weight"])).to(device=device, dtype=dtype))


def render_torch(source, tp, shape, background):
    """The pass as torch autograd sees it: source [elements, 3] (a texture flattened to [T T, 3]) -> image [V, H, W, 3]."""
    import torch
    colour = (tp["weight"][..., None] * source[tp["index"]]).sum(1)
    image = torch.as_tensor(np.asarray(background, np.float64), dtype=source.dtype, device=source.device) \
        .expand(int(np.prod(shape)), 3)
    return image.index_put((tp["pixel"],), colour).reshape(*shape, 3)


def pixel_weights(weights, masks, shape):
    """fit's weight of a pixel: weights[v] where the mask is non-zero, over 3 x their sum: [V, H, W, 1] float64."""
    V = shape[0]
    w = np.broadcast_to(np.ones(V) if weights is None else np.asarray(weights, np.float64), (V,))[:, None, None]
    w = np.broadcast_to(w, shape) * (1.0 if masks is None else (np.asarray(masks) != 0))
    return (w / (3.0 * w.sum()))[..., None]


def fit(start, tp, shape, background, target, pixel, iterations, lr, dtype):
    """mesh.fit_texture's loop on the restatement: torch's Adam on sum(pixel (render - target)^2), a clamp to [0, 1] after
    every step; returns (value [elements, 3], the loss before each step)."""
    import torch
    value = torch.as_tensor(np.asarray(start), dtype=dtype).clone().requires_grad_(True)
    target, pixel = torch.as_tensor(target, dtype=dtype), torch.as_tensor(pixel, dtype=dtype)
    optimiser = torch.optim.Adam([value], lr=lr)
    history = []
    for _ in range(iterations):
        optimiser.zero_grad(set_to_none=True)
        loss = (pixel * (render_torch(value, tp, shape, background) - target) ** 2).sum()
        loss.backward()
        optimiser.step()
        with torch.no_grad():
            value.clamp_(0.0, 1.0)
        history.append(float(loss.detach()))
    return value.detach(), history
