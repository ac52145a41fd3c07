"""Score network for the FFHQ config: an ADM-style U-Net in plain PyTorch-ROCm.

Out of scope as a kernel target (north_star keeps the score evaluations on PyTorch-ROCm; SURVEY.md
section 8 row a16) but needed to run and measure the hot path end to end.  The module tree and
parameter names follow guided_diffusion's checkpoint layout (`time_embed.0`, `input_blocks.k.0.in_layers.0`,
`...emb_layers.1`, `...out_layers.3`, `...skip_connection`, `k.1.norm/qkv/proj_out`, `middle_block`,
`output_blocks`, `out.0/out.2`) so that `models/ffhq_10m.pt` loads with `load_state_dict` unchanged
(reference: guided_diffusion/unet_ffhq.py:25-91 `create_model`, :467-734 `UNetModel`; config
configs/config_ffhq.yml:17-35).  When the checkpoint is absent the weights stay randomly initialised,
as in the reference's own fallback (unet_ffhq.py:87-90).
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels as K

FFHQ_CONFIG = dict(image_size=256, num_channels=128, num_res_blocks=1, channel_mult='', learn_sigma=True,
                   attention_resolutions='16', num_head_channels=64, use_scale_shift_norm=True,
                   resblock_updown=True)
_DEFAULT_MULT = {512: (0.5, 1, 1, 2, 2, 4, 4), 256: (1, 1, 2, 2, 4, 4), 128: (1, 1, 2, 3, 4), 64: (1, 2, 3, 4)}


def sinusoid_freqs(dim, max_period=10000):
    """Computed on the CPU exactly as the reference does (guided_diffusion/nn.py:114-116)."""
    half = dim // 2
    return torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32) / half)


def sinusoid(t, dim, freqs=None):
    freqs = sinusoid_freqs(dim).to(t.device) if freqs is None else freqs
    ang = t[:, None].float() * freqs[None]
    emb = torch.cat([ang.cos(), ang.sin()], dim=-1)
    return F.pad(emb, (0, dim % 2))


class _GroupNormAct(torch.autograd.Function):
    """y = act(GroupNorm(x + pre) (1 + scale) + shift) on the fused HIP kernels: 1 read + 1 write forward, 2 reads + 1 write
    for the input gradient on the one-pass kernels (csrc/gn_onepass.hip: a slab's statistics are exchanged between the
    workgroups that hold it in registers); 2 reads + 1 write / 4 reads + 1 write on the two-pass kernels (csrc/gn_act.hip),
    which serve the shapes the one-pass kernels do not cover or are not faster at (nhmc_gn_onepass_prefers) and
    NHMC_GN_ONEPASS=0.  Nothing but x is saved -- against
    5R + 4W / 7R + 3W for the ATen op sequence the reference's GroupNorm32 + scale-shift + SiLU lowers to
    (unet_ffhq.py:310-321)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, film, pre, groups, eps, act):
        xc = x if x.is_contiguous() else x.contiguous()
        y, ws, splits = K.gn_act_fwd(xc, gamma, beta, groups, eps, act, film, pre)
        ctx.save_for_backward(xc, gamma, beta, ws)
        ctx.consts = (film, pre)                              # constants of the path (no gradient flows into them)
        ctx.meta = (groups, eps, act, splits)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, gamma, beta, ws = ctx.saved_tensors
        groups, eps, act, splits = ctx.meta
        film, pre = ctx.consts
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx = K.gn_act_bwd(xc, dy, gamma, beta, groups, eps, act, film, ws, splits, pre)
        return dx, None, None, None, None, None, None, None


class _GroupNormActFork(torch.autograd.Function):
    """_GroupNormAct with x itself as a second output, for a block whose input feeds the GroupNorm AND the skip path
    (unet_ffhq.py:299-321: `h = self.in_layers(x)` ... `self.skip_connection(x) + h`).  The two gradients of x then meet
    inside the backward kernel (dx = fl(dx_groupnorm) + dx_skip, the bits of autograd's accumulation) instead of in a
    pass of their own."""

    @staticmethod
    def forward(ctx, x, gamma, beta, film, pre, groups, eps, act):
        xc = x if x.is_contiguous() else x.contiguous()
        y, ws, splits = K.gn_act_fwd(xc, gamma, beta, groups, eps, act, film, pre)
        ctx.save_for_backward(xc, gamma, beta, ws)
        ctx.consts = (film, pre)
        ctx.meta = (groups, eps, act, splits)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dx_skip):
        xc, gamma, beta, ws = ctx.saved_tensors
        groups, eps, act, splits = ctx.meta
        film, pre = ctx.consts
        if dy is None:
            return dx_skip, None, None, None, None, None, None, None
        dy = dy if dy.is_contiguous() else dy.contiguous()
        if dx_skip is not None and not dx_skip.is_contiguous():
            dx_skip = dx_skip.contiguous()
        dx = K.gn_act_bwd(xc, dy, gamma, beta, groups, eps, act, film, ws, splits, pre, add=dx_skip)
        return dx, None, None, None, None, None, None, None


class _GroupNormActCat(torch.autograd.Function):
    """_GroupNormActFork for a block input that arrives as two tensors, (h, skip) for cat([h, skip], dim=1) -- every
    output block of the U-Net (unet_ffhq.py:731 `th.cat([h, hs.pop()], dim=1)`).  The one-pass forward kernel reads the
    two sources and writes the concatenation (for the skip path's 1x1 convolution) next to y from the same load, so
    torch.cat's pass does not run; the backward writes the gradient as two contiguous tensors, so neither does the
    strided slicing of cat's backward nor the .contiguous() copies behind it."""

    @staticmethod
    def forward(ctx, h, skip, gamma, beta, groups, eps, act):
        hc, sc = h if h.is_contiguous() else h.contiguous(), skip if skip.is_contiguous() else skip.contiguous()
        y, ws, splits, x_cat = K.gn_act_fwd(hc, gamma, beta, groups, eps, act, x2=sc)
        ctx.save_for_backward(x_cat, gamma, beta, ws)
        ctx.meta = (groups, eps, act, splits, hc.shape[1])
        return y, x_cat

    @staticmethod
    def backward(ctx, dy, dx_skip):
        x_cat, gamma, beta, ws = ctx.saved_tensors
        groups, eps, act, splits, c1 = ctx.meta
        if dy is None:
            return dx_skip[:, :c1], dx_skip[:, c1:], None, None, None, None, None
        dy = dy if dy.is_contiguous() else dy.contiguous()
        if dx_skip is not None and not dx_skip.is_contiguous():
            dx_skip = dx_skip.contiguous()
        dh, dskip = K.gn_act_bwd(x_cat, dy, gamma, beta, groups, eps, act, None, ws, splits, add=dx_skip, c1=c1)
        return dh, dskip, None, None, None, None, None


class _BiasAdd2(torch.autograd.Function):
    """(h + bias_c) + other in one pass; the gradient reaches h and other unchanged."""

    @staticmethod
    def forward(ctx, h, bias, other):
        return K.bias_add2(h if h.is_contiguous() else h.contiguous(), bias, other if other.is_contiguous() else other.contiguous())

    @staticmethod
    def backward(ctx, g):
        return g, None, g


def fused_glue(x, *consts):
    """True when the HIP glue kernels serve this call: fp32 GPU activations whose spatial size is a multiple of 4 and
    constants (parameters, embedding terms) that carry no gradient; NHMC_FUSED_GN=0 keeps the ATen sequence (A/B runs)."""
    return x.is_cuda and x.dtype == torch.float32 and x[0, 0].numel() % 4 == 0 and os.environ.get('NHMC_FUSED_GN', '1') != '0' \
        and not any(c is not None and c.requires_grad for c in consts)


def group_norm_act(gn, x, act=True, film=None, act_fn=F.silu, pre=None):
    """GroupNorm `gn` of x (+ `pre`, a [C] or [B, C] term added first: the producing convolution's bias / an embedding
    term) (+ FiLM terms `film` = [B, 2C] scale | shift) (+ SiLU) of a score network.

    fp32 GPU tensors with frozen parameters -- the sampler's case -- run the fused HIP kernels; anything else (CPU
    tensors of the fixtures' side, float64 evaluation in the parity tests, parameters that require grad) is plain torch,
    as for any other module of this file -- with `act_fn` the activation in the reference's own form (nn.SiLU in the ADM
    U-Nets, x * sigmoid(x) in the VQ decoder)."""
    if fused_glue(x, gn.weight, gn.bias, film, pre):
        return _GroupNormAct.apply(x, gn.weight, gn.bias, film, pre, gn.num_groups, gn.eps, act)
    if pre is not None:
        x = x + pre.reshape(((1, -1) if pre.dim() == 1 else tuple(pre.shape)) + (1,) * (x.dim() - 2))
    h = F.group_norm(x, gn.num_groups, gn.weight, gn.bias, gn.eps)
    if film is not None:
        scale, shift = film.reshape(film.shape + (1,) * (x.dim() - 2)).chunk(2, dim=1)
        h = h * (1 + scale) + shift
    return act_fn(h) if act else h


def group_norm_act_fork(gn, x, act=True, act_fn=F.silu):
    """(group_norm_act(gn, x), x) for a block input that also feeds the block's skip path: on the fused kernels the
    second element is an alias of x whose gradient is added inside the GroupNorm's backward kernel."""
    if x.requires_grad and torch.is_grad_enabled() and fused_glue(x, gn.weight, gn.bias):
        return _GroupNormActFork.apply(x, gn.weight, gn.bias, None, None, gn.num_groups, gn.eps, act)
    return group_norm_act(gn, x, act=act, act_fn=act_fn), x


def pair_glue(gn, h, skip):
    """True when group_norm_act_pair runs on the two-source one-pass kernels."""
    return fused_glue(h, gn.weight, gn.bias) and skip.is_cuda and skip.dtype == h.dtype and skip.shape[2:] == h.shape[2:] \
        and K.gn_onepass_splits(h.shape[0], h.shape[1] + skip.shape[1], gn.num_groups, h[0, 0].numel()) > 0


def group_norm_act_pair(gn, h, skip, act=True, act_fn=F.silu):
    """group_norm_act_fork(gn, cat([h, skip], dim=1)) -> (y, x_cat) without torch.cat where the one-pass kernels cover the
    shape (_GroupNormActCat); the concatenation + the fork otherwise (CPU, float64, trainable parameters,
    NHMC_FUSED_GN=0, NHMC_GN_ONEPASS=0)."""
    if pair_glue(gn, h, skip):
        return _GroupNormActCat.apply(h, skip, gn.weight, gn.bias, gn.num_groups, gn.eps, act)
    return group_norm_act_fork(gn, torch.cat([h, skip], dim=1), act=act, act_fn=act_fn)


class _Conv3x3Wino(torch.autograd.Function):
    """A frozen 3x3 stride-1 padding-1 convolution (+ bias_k) (+ add) whose forward and / or backward-data pass runs on the
    Winograd MFMA kernel (csrc/wino_conv.hip); `route` = (forward, backward) says which.  A pass that is not routed runs
    the vendor library's kernel, as F.conv2d and its autograd node would.  Saves the filter only: there is no weight
    gradient, and the gradient reaches `add` unchanged.  `add_bias` (a routed forward only, conv_bias_add2_skip): `add` is a
    skip convolution's output without its bias, which the kernel's epilogue adds to it."""

    @staticmethod
    def forward(ctx, x, weight, bias, add, route, add_bias=None):
        xc = x if x.is_contiguous() else x.contiguous()
        if add is not None and not add.is_contiguous():
            add = add.contiguous()
        ctx.save_for_backward(weight)
        ctx.route_bwd, ctx.x_shape = route[1], tuple(x.shape)
        if route[0]:
            return K.conv3x3_wino(xc, weight, bias, add) if add_bias is None else K.conv3x3_wino_skip(xc, weight, bias, add, add_bias)
        if add is None:                                     # bias-only callers (conv_bias): the vendor kernel adds it
            return F.conv2d(xc, weight, bias, 1, 1)
        return K.bias_add2(F.conv2d(xc, weight, None, 1, 1), bias, add)

    @staticmethod
    def backward(ctx, g):
        (weight,) = ctx.saved_tensors
        dx = None
        if ctx.needs_input_grad[0]:
            gc = g if g.is_contiguous() else g.contiguous()
            dx = K.conv3x3_wino(gc, weight, backward=True) if ctx.route_bwd \
                else torch.nn.grad.conv2d_input(ctx.x_shape, weight, gc, 1, 1)
        return dx, None, None, (g if ctx.needs_input_grad[3] else None), None, None


def wino_route(conv, x, wino=None, up=False):
    """(forward, backward) routing of `conv` applied to x onto the Winograd MFMA kernel, or None when it stays F.conv2d:
    a frozen 3x3 stride-1 padding-1 convolution of fp32 GPU activations whose shape the kernel covers and, per direction,
    the library's measured table prefers (wino=True: wherever it is covered -- tests); NHMC_WINO=0 keeps the vendor library.
    up=True: the routing at twice x's resolution, for a convolution behind a nearest 2x upsample of x."""
    if wino is False or x.dim() != 4 or not fused_glue(x, conv.weight, conv.bias) or os.environ.get('NHMC_WINO', '1') == '0':
        return None
    if tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1) or conv.padding != (1, 1) \
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or conv.padding_mode != 'zeros':
        return None
    n, c, h, w = x.shape
    if up:
        h, w = 2 * h, 2 * w
    k = conv.out_channels
    fwd, bwd = K.conv3x3_wino_k32_covers(n, c, k, h, w), K.conv3x3_wino_k32_covers(n, k, c, h, w)
    if not wino:                                        # a shape is in one table only: k32's rows have k % 64 == 32
        fwd = fwd and (K.conv3x3_wino_prefers(0, n, c, k, h, w) or K.conv3x3_wino_k32_prefers(0, n, c, k, h, w))
        bwd = bwd and (K.conv3x3_wino_prefers(1, n, k, c, h, w) or K.conv3x3_wino_k32_prefers(1, n, k, c, h, w))
    bwd = bwd and x.requires_grad and torch.is_grad_enabled()
    return (fwd, bwd) if fwd or bwd else None


class _Conv3x3WinoUp(torch.autograd.Function):
    """conv(nearest 2x upsample of x), no bias, with the upsampled tensor never in memory: the Winograd kernel reads the
    low-res x (WINO_IN_UP) and skips the seven frequencies that are zero for such an input.  `pool`: the backward-data pass
    writes the 2 x 2 block sums of its output, the gradient of x, from its epilogue (WINO_OUT_POOL); otherwise the
    convolution's backward as in _Conv3x3Wino, then _Resample2x's."""

    @staticmethod
    def forward(ctx, x, weight, route_bwd, pool):
        xc = x if x.is_contiguous() else x.contiguous()
        ctx.save_for_backward(weight)
        ctx.route_bwd, ctx.pool, ctx.x_shape = route_bwd, pool, tuple(x.shape)
        return K.conv3x3_wino_up(xc, weight, K.WINO_IN_UP)

    @staticmethod
    def backward(ctx, g):
        (weight,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        gc = g if g.is_contiguous() else g.contiguous()
        if ctx.pool:
            return K.conv3x3_wino_up(gc, weight, K.WINO_OUT_POOL, backward=True), None, None, None
        B, C, h, w = ctx.x_shape
        full = K.conv3x3_wino(gc, weight, backward=True) if ctx.route_bwd \
            else torch.nn.grad.conv2d_input((B, C, 2 * h, 2 * w), weight, gc, 1, 1)
        return K.sr_H(full, 2).view(B, C, h, w).mul_(4.0), None, None, None


class _Conv3x3WinoAddUp(torch.autograd.Function):
    """_Conv3x3Wino with the forward pass on the kernel and `add` at half the resolution, standing for its nearest 2x
    upsample (WINO_ADD_UP): the residual of an up-sampling ResBlock.  The gradient reaches `add` as _Resample2x's backward
    would form it, 4 x the 2 x 2 block means."""

    @staticmethod
    def forward(ctx, x, weight, bias, add, route_bwd):
        xc = x if x.is_contiguous() else x.contiguous()
        ctx.save_for_backward(weight)
        ctx.route_bwd, ctx.x_shape, ctx.add_shape = route_bwd, tuple(x.shape), tuple(add.shape)
        return K.conv3x3_wino(xc, weight, bias, add if add.is_contiguous() else add.contiguous())    # low-res add: ADD_UP

    @staticmethod
    def backward(ctx, g):
        (weight,) = ctx.saved_tensors
        gc = g if g.is_contiguous() else g.contiguous()
        dx = dadd = None
        if ctx.needs_input_grad[0]:
            dx = K.conv3x3_wino(gc, weight, backward=True) if ctx.route_bwd \
                else torch.nn.grad.conv2d_input(ctx.x_shape, weight, gc, 1, 1)
        if ctx.needs_input_grad[3]:
            dadd = K.sr_H(gc, 2).view(ctx.add_shape).mul_(4.0)
        return dx, None, None, dadd, None


class _Conv3x3Thin(torch.autograd.Function):
    """A frozen 3x3 stride-1 padding-1 convolution (+ bias_k) with a thin side (at most 8 channels) whose forward and / or
    backward-data pass runs on the direct packed-FMA kernels (csrc/thin_conv.hip); `route` = (forward, backward) says which.
    The pass whose input is thin (forward of 3 -> 128, backward-data of 128 -> 6) runs the thin-input kernel, the other one
    the thin-output kernel.  A pass that is not routed is the vendor library's call, as F.conv2d and its autograd node make
    it.  Saves the filter only: there is no weight gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, route):
        xc = x if x.is_contiguous() else x.contiguous()
        ctx.save_for_backward(weight)
        ctx.route_bwd, ctx.x_shape = route[1], tuple(x.shape)
        if not route[0]:
            return F.conv2d(xc, weight, bias, 1, 1)
        return (K.conv3x3_thin_in if weight.shape[1] <= 8 else K.conv3x3_thin_out)(xc, weight, bias)

    @staticmethod
    def backward(ctx, g):
        (weight,) = ctx.saved_tensors
        dx = None
        if ctx.needs_input_grad[0]:
            gc = g if g.is_contiguous() else g.contiguous()
            dx = (K.conv3x3_thin_in if weight.shape[0] <= 8 else K.conv3x3_thin_out)(gc, weight, backward=True) if ctx.route_bwd \
                else torch.nn.grad.conv2d_input(ctx.x_shape, weight, gc, 1, 1)
        return dx, None, None, None


def thin_route(conv, x, thin=None):
    """(forward, backward) routing of `conv` applied to x onto the thin kernels, or None when the module call stays: a
    frozen 3x3 stride-1 padding-1 convolution of fp32 GPU activations with at most 8 channels on one side and a multiple of
    32 on the other, each direction where the kernel that serves it covers the shape and the library's measured table
    prefers it (thin=True: wherever it is covered -- tests).  NHMC_THIN_CONV=0, read per call, keeps the vendor library."""
    if thin is False or x.dim() != 4 or not fused_glue(x, conv.weight, conv.bias) or os.environ.get('NHMC_THIN_CONV', '1') == '0':
        return None
    if tuple(conv.kernel_size) != (3, 3) or tuple(conv.stride) != (1, 1) or conv.padding != (1, 1) \
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or conv.padding_mode != 'zeros':
        return None
    n, c, h, w = x.shape
    k = conv.out_channels
    if c <= 8:                                          # thin -> wide: thin-input forward, thin-output backward-data
        fwd, bwd = K.conv3x3_thin_in_covers(n, c, k, h, w), K.conv3x3_thin_out_covers(n, k, c, h, w)
        if not thin:
            fwd, bwd = fwd and K.conv3x3_thin_in_prefers(0, n, c, k, h, w), bwd and K.conv3x3_thin_out_prefers(1, n, k, c, h, w)
    else:
        fwd, bwd = K.conv3x3_thin_out_covers(n, c, k, h, w), K.conv3x3_thin_in_covers(n, k, c, h, w)
        if not thin:
            fwd, bwd = fwd and K.conv3x3_thin_out_prefers(0, n, c, k, h, w), bwd and K.conv3x3_thin_in_prefers(1, n, k, c, h, w)
    bwd = bwd and x.requires_grad and torch.is_grad_enabled()
    return (fwd, bwd) if fwd or bwd else None


def conv_thin(conv, x, thin=None):
    """conv(x) for the network's first and last convolution: on the thin kernels where thin_route says so, the plain
    module call otherwise."""
    route = thin_route(conv, x, thin)
    if route is not None:
        return _Conv3x3Thin.apply(x, conv.weight, conv.bias, route)
    return conv(x)


def conv_nobias(conv, x, wino=None):
    """The convolution without its bias (the fused glue adds it where the output is consumed)."""
    route = wino_route(conv, x, wino)
    if route is not None:
        return _Conv3x3Wino.apply(x, conv.weight, None, None, route)
    return F.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)


def conv_bias(conv, x, wino=None):
    """conv(x) with its bias and no residual (the convolution behind an upsample): the bias is added in the Winograd
    kernel's epilogue where that takes the forward pass, by the vendor library's convolution otherwise."""
    route = wino_route(conv, x, wino)
    if route is not None:
        return _Conv3x3Wino.apply(x, conv.weight, conv.bias, None, route)
    return F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups)


def conv_bias_add2(conv, x, other, wino=None):
    """(conv(x) + bias) + other: the residual add of a ResBlock, inside the convolution's epilogue where the Winograd kernel
    takes the forward pass, on k_bias_add2 behind the convolution otherwise."""
    route = wino_route(conv, x, wino)
    if route is not None and route[0]:
        return _Conv3x3Wino.apply(x, conv.weight, conv.bias, other, route)
    return _BiasAdd2.apply(conv_nobias(conv, x, wino), conv.bias, other)


def conv_bias_add2_skip(conv, x, skip, sx, wino=None):
    """conv_bias_add2(conv, x, skip(sx)) for a ResBlock's skip path `skip`.  Where that is a frozen 1x1 convolution with a
    bias and `conv`'s forward pass runs on the eight-wave Winograd kernel, the skip convolution runs without its bias and
    the kernel's epilogue adds it, (acc + bias) + (skip + skip_bias): the vendor path's broadcast pass over the skip
    tensor (`output.add_(bias)` behind its GEMM) computed the same inner fp32 add, so the bits are unchanged and the pass
    is gone.  NHMC_SKIP_BIAS=0 (read per call) keeps the pass; so do the narrow geometries, four waves and k_bias_add2."""
    route = wino_route(conv, x, wino)
    if route is not None and route[0] and isinstance(skip, nn.Conv2d) and skip.bias is not None \
            and tuple(skip.kernel_size) == (1, 1) and tuple(skip.stride) == (1, 1) and skip.padding == (0, 0) \
            and tuple(skip.dilation) == (1, 1) and skip.groups == 1 and skip.out_channels == conv.out_channels \
            and fused_glue(sx, skip.weight, skip.bias) and sx.shape[2:] == x.shape[2:] \
            and K.conv3x3_wino_skip_covers(x.shape[0], x.shape[1], conv.out_channels, x.shape[2], x.shape[3]):
        return _Conv3x3Wino.apply(x, conv.weight, conv.bias, F.conv2d(sx, skip.weight, None), route, skip.bias)
    return conv_bias_add2(conv, x, skip(sx), wino)


class _Resample2x(torch.autograd.Function):
    """2x2 average pool / nearest 2x upsample on the block-mean kernels of the SR operator (csrc/data_term.hip: `k_sr`
    with ratio 2 is exactly this pair, H = block mean and H^T = broadcast x scale): each is the other's backward, so
    ATen's slow avg_pool2d_backward (429 us per call at the U-Net's sizes) never runs."""

    @staticmethod
    def forward(ctx, x, up):
        B, C, d = x.shape[0], x.shape[1], x.shape[2]
        ctx.up, ctx.dims = up, (B, C, d)
        xc = x if x.is_contiguous() else x.contiguous()
        if up:
            return K.sr_Ht(xc.reshape(B, -1), 2, C, 2 * d, 1.0).view(B, C, 2 * d, 2 * d)
        return K.sr_H(xc, 2).view(B, C, d // 2, d // 2)

    @staticmethod
    def backward(ctx, g):
        B, C, d = ctx.dims
        gc = g if g.is_contiguous() else g.contiguous()
        if ctx.up:                                          # sum over each 2x2 block = 4 x its mean
            return K.sr_H(gc, 2).view(B, C, d, d).mul_(4.0), None
        return K.sr_Ht(gc.reshape(B, -1), 2, C, d, 0.25).view(B, C, d, d), None


class Resample(nn.Module):
    """Parameter-free 2x nearest upsample / 2x2 average pool (the reference's conv-less up/down)."""

    def __init__(self, up):
        super().__init__()
        self.up = up

    def on_kernels(self, x):
        """True when x is resampled by the block-mean kernels (_Resample2x)."""
        return fused_glue(x) and x.dim() == 4 and x.shape[2] == x.shape[3] and x.shape[0] <= 65535 \
            and (x.shape[2] % 8 == 0 or (self.up and x.shape[2] % 2 == 0))

    def forward(self, x):
        if self.on_kernels(x):
            return _Resample2x.apply(x, self.up)
        return F.interpolate(x, scale_factor=2, mode='nearest') if self.up else F.avg_pool2d(x, 2)


class ResBlock(nn.Module):
    takes_emb = True
    wino = None              # routing of the two 3x3 convolutions (wino_route): None = the measured table, True = forced (tests)

    def __init__(self, ch, emb_ch, out_ch=None, up=False, down=False):
        super().__init__()
        out_ch = out_ch or ch
        self.in_layers = nn.Sequential(nn.GroupNorm(32, ch), nn.SiLU(), nn.Conv2d(ch, out_ch, 3, padding=1))
        self.resample, self.up = up or down, up
        self.h_upd = self.x_upd = Resample(up) if self.resample else nn.Identity()
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_ch, 2 * out_ch))
        self.out_layers = nn.Sequential(nn.GroupNorm(32, out_ch), nn.SiLU(), nn.Identity(),
                                        nn.Conv2d(out_ch, out_ch, 3, padding=1))
        self.skip_connection = nn.Identity() if out_ch == ch else nn.Conv2d(ch, out_ch, 1)

    def up_routes(self, h, x):
        """An up-sampling block whose two upsamples fold into its convolutions (csrc/wino_conv.hip, "Nearest 2x upsample"):
        ((forward, backward, pooled backward) of conv1, (forward, backward) of conv2), or None for the materialised path.
        Both forward passes must be routed to the wide Winograd kernel at the upsampled shape, on eight waves
        (NHMC_WINO_WAVES) and with NHMC_WINO_UP not 0 (both read per call); the skip path must be the identity; h and x
        must be what the block-mean kernels would upsample."""
        conv1, conv2 = self.in_layers[2], self.out_layers[3]
        if not isinstance(self.skip_connection, nn.Identity) or not self.h_upd.on_kernels(h) or not self.x_upd.on_kernels(x) \
                or x.shape != h.shape or not fused_glue(h, conv1.bias, conv2.bias):
            return None
        n, c, k, hh, ww = h.shape[0], conv1.in_channels, conv1.out_channels, 2 * h.shape[2], 2 * h.shape[3]
        r1, r2 = wino_route(conv1, h, self.wino, up=True), wino_route(conv2, h, self.wino, up=True)
        if r1 is None or r2 is None or not r1[0] or not r2[0] or conv2.in_channels != k \
                or not K.conv3x3_wino_up_covers(n, c, k, hh, ww) or not K.conv3x3_wino_up_covers(n, k, k, hh, ww):
            return None
        return (True, r1[1], r1[1] and K.conv3x3_wino_up_covers(n, k, c, hh, ww)), (True, r2[1])

    def forward(self, x, emb):
        """x: the block input, or a pair (h, skip) standing for cat([h, skip], dim=1) (the output blocks)."""
        if isinstance(x, tuple):
            h, x = group_norm_act_pair(self.in_layers[0], *x)
        else:
            h, x = group_norm_act_fork(self.in_layers[0], x)             # GroupNorm + SiLU; x goes on to the skip path
        up = self.up_routes(h, x) if self.up else None
        if self.resample and up is None:
            h, x = self.h_upd(h), self.x_upd(x)
        conv1, conv2, film = self.in_layers[2], self.out_layers[3], self.emb_layers(emb)
        if up is not None and not fused_glue(h, conv1.bias, conv2.bias, film):
            h, x, up = self.h_upd(h), self.x_upd(x), None
        if up is not None:
            # the upsampled h and x never reach memory: conv1 reads the low-res h, conv2's epilogue adds the low-res x
            (_, bwd1, pool), (_, bwd2) = up
            h = group_norm_act(self.out_layers[0], _Conv3x3WinoUp.apply(h, conv1.weight, bwd1, pool), film=film, pre=conv1.bias)
            return _Conv3x3WinoAddUp.apply(h, conv2.weight, conv2.bias, x, bwd2)
        if fused_glue(h, conv1.bias, conv2.bias, film):
            # the two convolutions run without their broadcast bias passes: conv1's bias enters the next GroupNorm's
            # load, conv2's the residual add
            h = group_norm_act(self.out_layers[0], conv_nobias(conv1, h, self.wino), film=film, pre=conv1.bias)
            return conv_bias_add2_skip(conv2, h, self.skip_connection, x, self.wino)
        h = group_norm_act(self.out_layers[0], conv1(h), film=film)      # scale-shift norm (FiLM) + SiLU
        return self.skip_connection(x) + conv2(h)


class AttentionBlock(nn.Module):
    takes_emb = False

    def __init__(self, ch, head_ch):
        super().__init__()
        self.heads = ch // head_ch
        self.norm = nn.GroupNorm(32, ch)
        self.qkv = nn.Conv1d(ch, 3 * ch, 1)
        self.proj_out = nn.Conv1d(ch, ch, 1)

    def forward(self, x):
        b, c, hh, ww = x.shape
        x = x.reshape(b, c, -1)
        qkv = self.qkv(group_norm_act(self.norm, x, act=False))
        # "legacy" order: heads are split before q/k/v
        q, k, v = qkv.reshape(b * self.heads, 3 * c // self.heads, -1).split(c // self.heads, dim=1)
        s = 1 / math.sqrt(math.sqrt(c // self.heads))
        w = torch.softmax(torch.einsum('bct,bcs->bts', q * s, k * s), dim=-1)
        h = torch.einsum('bts,bcs->bct', w, v).reshape(b, c, -1)
        return (x + self.proj_out(h)).reshape(b, c, hh, ww)


class Stage(nn.Sequential):
    def forward(self, x, emb):
        for layer in self:
            if isinstance(layer, nn.Conv2d):                    # input_blocks[0]: the network's first, thin convolution
                x = conv_thin(layer, x)
            else:
                x = layer(x, emb) if getattr(layer, 'takes_emb', False) else layer(x)
        return x


class UNetModel(nn.Module):
    def __init__(self, image_size=256, in_channels=3, model_channels=128, out_channels=6, num_res_blocks=1,
                 attention_ds=(16,), channel_mult=(1, 1, 2, 2, 4, 4), num_head_channels=64):
        super().__init__()
        self.model_channels = mc = model_channels
        emb = 4 * mc
        self.time_embed = nn.Sequential(nn.Linear(mc, emb), nn.SiLU(), nn.Linear(emb, emb))
        # resident copy of the embedding frequencies (not a checkpoint key): no host->device copy per call, which also
        # keeps the forward capturable into a hipGraph
        self.register_buffer('_freqs', sinusoid_freqs(mc), persistent=False)
        ch = int(channel_mult[0] * mc)
        self.input_blocks = nn.ModuleList([Stage(nn.Conv2d(in_channels, ch, 3, padding=1))])
        skip_chs, ds = [ch], 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, emb, int(mult * mc))]
                ch = int(mult * mc)
                if ds in attention_ds:
                    layers.append(AttentionBlock(ch, num_head_channels))
                self.input_blocks.append(Stage(*layers))
                skip_chs.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(Stage(ResBlock(ch, emb, ch, down=True)))
                skip_chs.append(ch)
                ds *= 2
        self.middle_block = Stage(ResBlock(ch, emb), AttentionBlock(ch, num_head_channels), ResBlock(ch, emb))
        self.output_blocks = nn.ModuleList()
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                layers = [ResBlock(ch + skip_chs.pop(), emb, int(mc * mult))]
                ch = int(mc * mult)
                if ds in attention_ds:
                    layers.append(AttentionBlock(ch, num_head_channels))
                if level and i == num_res_blocks:
                    layers.append(ResBlock(ch, emb, ch, up=True))
                    ds //= 2
                self.output_blocks.append(Stage(*layers))
        self.out = nn.Sequential(nn.GroupNorm(32, ch), nn.SiLU(), nn.Conv2d(ch, out_channels, 3, padding=1))

    def forward(self, x, timesteps, y=None):
        emb = self.time_embed(sinusoid(timesteps, self.model_channels, self._freqs))
        hs, h = [], x
        for blk in self.input_blocks:
            h = blk(h, emb)
            hs.append(h)
        h = self.middle_block(h, emb)
        for blk in self.output_blocks:
            # the pair goes to the block's first GroupNorm kernel, which forms the concatenation as a by-product
            h = blk((h, hs.pop()) if fused_glue(h) else torch.cat([h, hs.pop()], dim=1), emb)
        return conv_thin(self.out[2], group_norm_act(self.out[0], h))


def create_model(image_size=256, num_channels=128, num_res_blocks=1, channel_mult='', learn_sigma=True,
                 class_cond=False, use_checkpoint=False, attention_resolutions='16', num_heads=4,
                 num_head_channels=64, num_heads_upsample=-1, use_scale_shift_norm=True, dropout=0.0,
                 resblock_updown=True, use_fp16=False, use_new_attention_order=False, model_path=''):
    """Keyword-compatible with the reference factory (unet_ffhq.py:25-91) for the options the FFHQ
    config uses; anything that would change the architecture away from it is rejected loudly."""
    if class_cond or use_fp16 or use_new_attention_order or not use_scale_shift_norm or not resblock_updown \
            or num_head_channels <= 0 or dropout:
        raise NotImplementedError('only the FFHQ-config architecture variant is built here')
    mult = _DEFAULT_MULT[image_size] if channel_mult == '' else tuple(int(c) for c in str(channel_mult).split(','))
    att = tuple(image_size // int(r) for r in str(attention_resolutions).split(','))
    model = UNetModel(image_size, 3, num_channels, 6 if learn_sigma else 3, num_res_blocks, att, mult, num_head_channels)
    import os
    if model_path and os.path.exists(model_path):
        model.load_state_dict(torch.load(model_path, map_location='cpu', weights_only=True))
    elif model_path:
        print(f'checkpoint {model_path} not found / randomly initialised')
    return model


def conv3x3_shapes(config=None):
    """[(C, K, resolution, count)] of every 3x3 stride-1 padding-1 Conv2d call of one forward pass of create_model(**config)
    (default FFHQ_CONFIG) on a [1, 3, image_size, image_size] input, ordered by falling resolution, then C, then K.
    Found by running the model on the `meta` device with a forward hook on every Conv2d: meta tensors take the unfused
    path, so each convolution is a module call, and nothing is allocated or computed.  The routing table of the Winograd
    kernel and tools/conv_bench.py rest on this list."""
    config = dict(FFHQ_CONFIG if config is None else config)
    with torch.device('meta'):
        model = create_model(**config)
    seen, hooks = {}, []

    def hook(mod, args, out):
        key = (mod.in_channels, mod.out_channels, args[0].shape[-1])
        seen[key] = seen.get(key, 0) + 1
    for mod in model.modules():
        if isinstance(mod, nn.Conv2d) and tuple(mod.kernel_size) == (3, 3) and tuple(mod.stride) == (1, 1) \
                and mod.padding == (1, 1):
            hooks.append(mod.register_forward_hook(hook))
    size = config.get('image_size', 256)
    with torch.no_grad():
        model(torch.empty(1, 3, size, size, device='meta'), torch.zeros(1, device='meta'))
    for h in hooks:
        h.remove()
    return [(c, k, res, n) for (c, k, res), n in sorted(seen.items(), key=lambda kv: (-kv[0][2], kv[0][0], kv[0][1]))]
