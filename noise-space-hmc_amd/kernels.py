"""Typed torch-tensor front ends of the C ABI (include/nhmc.h).

torch is plumbing here: it owns device memory and the stream; every function below checks its
operands (device, dtype, contiguity, shape) on the host, then hands raw pointers to libnhmc.so on
the CURRENT torch stream.  No function allocates inside the library; outputs are torch tensors
created here.  Nothing falls back to torch arithmetic.
"""
import ctypes as C
import os

import torch

from . import _lib

LF_FIRST, LF_MID, LF_LAST = 0, 1, 2


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, dtype=None, name='tensor', contiguous=True):
    """The checked pointer of an operand (None -> null).  contiguous=False: a strided view whose strides the caller has
    checked and hands to the library."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise _lib.NhmcError(f'{name} must live on the GPU (got {t.device}); libnhmc has no CPU path')
    if dtype is not None and t.dtype != dtype:
        raise _lib.NhmcError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous() and contiguous:
        raise _lib.NhmcError(f'{name} must be contiguous')
    return C.c_void_p(t.data_ptr())


def _chains_elems(x):
    return x.shape[0], x[0].numel()


def _f64(v, n, device):
    """per-chain fp64 scalars: python float / sequence / tensor -> device double[n]"""
    if isinstance(v, torch.Tensor):
        if v.dtype != torch.float64 or v.numel() != n:
            raise _lib.NhmcError('per-chain scalar tensors must be float64 of length n_chains')
        return v
    return torch.full((n,), float(v), dtype=torch.float64, device=device) if not hasattr(v, '__len__') \
        else torch.tensor(list(v), dtype=torch.float64, device=device)


# ---- a1-a4 ----------------------------------------------------------------------------------
def leapfrog_tiles(n_elem):
    return _lib.load().nhmc_leapfrog_tiles(n_elem)


def leapfrog_ws(n_chains, n_elem, device):
    return torch.empty(n_chains * leapfrog_tiles(n_elem) * 2, dtype=torch.float64, device=device)


def _sums_ws(sums_ws, B, N):
    """The checked pointer of a leapfrog sums workspace (leapfrog_ws(B, N, device))."""
    if sums_ws is None or sums_ws.numel() < B * leapfrog_tiles(N) * 2:
        raise _lib.NhmcError('sums_ws missing or too small')
    return _p(sums_ws, torch.float64, 'sums_ws')


def leapfrog_fused(mode, x, p, g, eps, sigma_y, m_inv, sums_ws=None, g2=None):
    """In place on x, p.  eps / sigma_y: float64 device tensors [B] (or python floats)."""
    lib = _lib.load()
    B, N = _chains_elems(x)
    if p.shape != x.shape or g.shape != x.shape or (g2 is not None and g2.shape != x.shape):
        raise _lib.NhmcError('x, p, g (and g2) must have the same shape')
    eps, sigma_y = _f64(eps, B, x.device), _f64(sigma_y, B, x.device)
    if mode != LF_MID and sums_ws is None:
        raise _lib.NhmcError('FIRST/LAST modes need sums_ws')
    if sums_ws is not None and sums_ws.numel() < B * leapfrog_tiles(N) * 2:
        raise _lib.NhmcError('sums_ws too small')
    rc = lib.nhmc_leapfrog_fused(mode, _p(x, torch.float32, 'x'), _p(p, torch.float32, 'p'),
                                 _p(g, torch.float32, 'g'), _p(g2, torch.float32, 'g2'),
                                 _p(eps, torch.float64, 'eps'), _p(sigma_y, torch.float64, 'sigma_y'),
                                 float(m_inv), B, N, _p(sums_ws, torch.float64, 'sums_ws'), _stream())
    _lib.check(rc, 'nhmc_leapfrog_fused')


def leapfrog_first(x_in, x_out, p, g, eps, sigma_y, m_inv, sums_ws, g2=None):
    """FIRST mode out of place in x: x_out <- proposal position, x_in untouched, p updated in place."""
    lib = _lib.load()
    B, N = _chains_elems(x_in)
    if x_out.shape != x_in.shape or p.shape != x_in.shape or g.shape != x_in.shape or (g2 is not None and g2.shape != x_in.shape):
        raise _lib.NhmcError('x_in, x_out, p, g (and g2) must have the same shape')
    if x_out.data_ptr() == x_in.data_ptr():
        raise _lib.NhmcError('leapfrog_first is out of place: x_out must not alias x_in')
    eps, sigma_y = _f64(eps, B, x_in.device), _f64(sigma_y, B, x_in.device)
    rc = lib.nhmc_leapfrog_first(_p(x_in, torch.float32, 'x_in'), _p(x_out, torch.float32, 'x_out'), _p(p, torch.float32, 'p'),
                                 _p(g, torch.float32, 'g'), _p(g2, torch.float32, 'g2'), _p(eps, torch.float64, 'eps'),
                                 _p(sigma_y, torch.float64, 'sigma_y'), float(m_inv), B, N, _sums_ws(sums_ws, B, N), _stream())
    _lib.check(rc, 'nhmc_leapfrog_first')


# ---- gradient cache (nhmc.h "Gradient cache") -------------------------------------------------
def _g_pair(g_pair, sel, B, N):
    """g_pair: a [2, B_total, ...] float32 tensor or a [:, lo:hi] view of one; sel int32 [B].
    -> (g_pair pointer, sel pointer, pair_stride in elements)"""
    if g_pair.dim() < 2 or g_pair.shape[0] != 2 or g_pair.shape[1] != B or g_pair[0, 0].numel() != N:
        raise _lib.NhmcError(f'g_pair must be [2, {B}, ...] with {N} elements per chain, got {tuple(g_pair.shape)}')
    if not g_pair[0].is_contiguous():
        raise _lib.NhmcError('g_pair: each slot must be contiguous')
    if sel.numel() != B:
        raise _lib.NhmcError('sel must be int32 [n_chains]')
    return _p(g_pair, torch.float32, 'g_pair', contiguous=False), _p(sel, torch.int32, 'sel'), g_pair.stride(0)


def _loss_pair(loss_pair, B):
    """loss_pair: float64 [2, B_total] or a [:, lo:hi] view of one -> (pointer, stride in elements)"""
    if loss_pair.shape != (2, B) or loss_pair.stride(1) != 1:
        raise _lib.NhmcError('loss_pair must be float64 [2, n_chains] (or a [:, lo:hi] view)')
    return _p(loss_pair, torch.float64, 'loss_pair', contiguous=False), loss_pair.stride(0)


def grad_cache_store(g, g2, loss, g_pair, loss_pair, sel, flip=0):
    """slot (sel ^ flip) of every chain <- (g + g2, loss)"""
    lib = _lib.load()
    B, N = _chains_elems(g)
    gp, sp, ps = _g_pair(g_pair, sel, B, N)
    lp, ls = _loss_pair(loss_pair, B)
    if g2 is not None and g2.shape != g.shape:
        raise _lib.NhmcError('g and g2 must have the same shape')
    rc = lib.nhmc_grad_cache_store(_p(g, torch.float32, 'g'), _p(g2, torch.float32, 'g2'), _p(loss, torch.float64, 'loss'),
                                   gp, lp, sp, int(flip), ps, ls, B, N, _stream())
    _lib.check(rc, 'nhmc_grad_cache_store')


def leapfrog_first_cached(x_in, x_out, p, g_pair, sel, eps, sigma_y, m_inv, sums_ws):
    """FIRST half step (out of place in x) with the gradient read from the cache slot sel[chain]."""
    lib = _lib.load()
    B, N = _chains_elems(x_in)
    if x_out.shape != x_in.shape or p.shape != x_in.shape:
        raise _lib.NhmcError('x_in, x_out, p must have the same shape')
    gp, sp, ps = _g_pair(g_pair, sel, B, N)
    eps, sigma_y = _f64(eps, B, x_in.device), _f64(sigma_y, B, x_in.device)
    rc = lib.nhmc_leapfrog_first_cached(_p(x_in, torch.float32, 'x_in'), _p(x_out, torch.float32, 'x_out'),
                                        _p(p, torch.float32, 'p'), gp, sp, ps, _p(eps, torch.float64), _p(sigma_y, torch.float64),
                                        float(m_inv), B, N, _sums_ws(sums_ws, B, N), _stream())
    _lib.check(rc, 'nhmc_leapfrog_first_cached')


def leapfrog_last_cached(x, p, g, g2, g_pair, loss_pair, sel, loss, eps, sigma_y, m_inv, sums_ws):
    """LAST step; slot 1 - sel[chain] <- (g + g2, loss) of the trajectory's end point."""
    lib = _lib.load()
    B, N = _chains_elems(x)
    if p.shape != x.shape or g.shape != x.shape or (g2 is not None and g2.shape != x.shape):
        raise _lib.NhmcError('x, p, g (and g2) must have the same shape')
    gp, sp, ps = _g_pair(g_pair, sel, B, N)
    lp, ls = _loss_pair(loss_pair, B)
    eps, sigma_y = _f64(eps, B, x.device), _f64(sigma_y, B, x.device)
    if loss.numel() != B:
        raise _lib.NhmcError('loss must have one entry per chain')
    rc = lib.nhmc_leapfrog_last_cached(_p(x, torch.float32, 'x'), _p(p, torch.float32, 'p'), _p(g, torch.float32, 'g'),
                                       _p(g2, torch.float32, 'g2'), gp, sp, ps, _p(loss, torch.float64, 'loss'), lp, ls,
                                       _p(eps, torch.float64), _p(sigma_y, torch.float64), float(m_inv), B, N,
                                       _sums_ws(sums_ws, B, N), _stream())
    _lib.check(rc, 'nhmc_leapfrog_last_cached')


def grad_cache_flip(accept, sel):
    lib = _lib.load()
    _lib.check(lib.nhmc_grad_cache_flip(_p(accept, torch.int32, 'accept'), _p(sel, torch.int32, 'sel'), sel.numel(), _stream()),
               'nhmc_grad_cache_flip')


# ---- a9-a11 ---------------------------------------------------------------------------------
def _mix_shapes(xt, e):
    B, Cc = xt.shape[0], xt.shape[1]
    hw = xt[0, 0].numel()
    if e.shape[0] != B or e.shape[2:] != xt.shape[2:]:
        raise _lib.NhmcError(f'score output shape {tuple(e.shape)} does not match xt {tuple(xt.shape)}')
    return B, Cc, hw, e.shape[1]


def _alpha(a, B, device):
    if a.dim() == 1 and a.numel() == B and a.dtype == torch.float32 and a.device == device and a.is_contiguous():
        return a                                     # already the per-chain array the kernels take (engine's cached tables)
    a = a.reshape(-1)
    if a.numel() == 1 and B > 1:
        a = a.expand(B)
    if a.numel() != B:
        raise _lib.NhmcError('alpha-bar must have one entry per chain')
    return a.to(device=device, dtype=torch.float32).contiguous()


def _last_vjp_io(xt, e, at, at_next, g_e_out, fills_sigma):
    """What every fused "data term + last DDIM-step VJP" wrapper starts with -> (dims, mix, grads, outs, alphas):
        dims    (B, C, hw): the chunk's chains, channels and pixels per plane
        mix     the five mix arguments in ABI order: xt, e, e_channels, at, at_next
        grads   the gradient outputs in ABI order: g_xt, g_e (and fill_sigma when the entry takes it)
        outs    (g_xt, g_e): the tensors behind `grads`, which the wrapper returns after its loss
        alphas  the alpha-bar arrays behind `mix`: the caller holds them until after its launch call (see ddim_map_back)
    fills_sigma: the kernel zero-fills the learned-sigma half of a fresh g_e itself (its fill_sigma argument); the others
    write channels [0, C) only and get a zeroed one.  A caller's g_e_out is checked before anything is allocated or launched."""
    B, Cc, hw, ec = _mix_shapes(xt, e)
    if g_e_out is not None and g_e_out.shape != e.shape:
        raise _lib.NhmcError(f'g_e_out must have the shape of the score output {tuple(e.shape)}, got {tuple(g_e_out.shape)}')
    at, at_next = _alpha(at, B, xt.device), _alpha(at_next, B, xt.device)
    mix = (_p(xt, torch.float32, 'xt'), _p(e, torch.float32, 'e'), ec, _p(at), _p(at_next))
    g_xt = torch.empty_like(xt)
    g_e = g_e_out if g_e_out is not None else (torch.empty_like(e) if fills_sigma else torch.zeros_like(e))
    grads = (_p(g_xt), _p(g_e, torch.float32, 'g_e'), int(g_e_out is None)) if fills_sigma else (_p(g_xt), _p(g_e, torch.float32, 'g_e'))
    return (B, Cc, hw), mix, grads, (g_xt, g_e), (at, at_next)


def ddim_mix_fwd(xt, e, at, at_next, final_clip=False, want=('xt_next',), out=None):
    """Returns a dict with the requested outputs among 'xt_next', 'x0_t', 'add_up'.  out: tensor to write xt_next into."""
    lib = _lib.load()
    B, Cc, hw, ec = _mix_shapes(xt, e)
    at, at_next = _alpha(at, B, xt.device), _alpha(at_next, B, xt.device)
    if out is not None and (out.shape != xt.shape or 'xt_next' not in want):
        raise _lib.NhmcError('ddim_mix_fwd: out must have the shape of xt and xt_next must be wanted')
    out = {k: (out if (k == 'xt_next' and out is not None) else torch.empty_like(xt)) for k in want}
    rc = lib.nhmc_ddim_mix_fwd(_p(xt, torch.float32, 'xt'), _p(e, torch.float32, 'e'), ec, _p(at), _p(at_next),
                               int(final_clip), _p(out.get('xt_next')), _p(out.get('x0_t')), _p(out.get('add_up')),
                               B, Cc, hw, _stream())
    _lib.check(rc, 'nhmc_ddim_mix_fwd')
    return out


def ddim_map_back(x0_t, add_up, at_next):
    lib = _lib.load()
    B, N = _chains_elems(x0_t)
    out = torch.empty_like(x0_t)
    an = _alpha(at_next, B, x0_t.device)                 # keep temporaries alive until after the launch call:
    rc = lib.nhmc_ddim_map_back(_p(x0_t, torch.float32, 'x0_t'), _p(add_up, torch.float32, 'add_up'),   # a freed block
                                _p(an), _p(out), B, N, _stream())                                          # can be re-issued
    _lib.check(rc, 'nhmc_ddim_map_back')
    return out


def ddim_mix_bwd(gout, xt, e, at, at_next, final_clip=False, gout2=None, g_x0=None, g_e_out=None, want_g_e=True):
    """-> (g_xt [B,C,H,W], g_e [B,e_channels,H,W]).  g_x0: split form (gout is then d/d add_up).
    g_e_out: a persistent buffer whose sigma-channels are already zero (they are then not rewritten).
    want_g_e=False: the score carries no gradient; g_e is not formed (returned as None)."""
    lib = _lib.load()
    B, Cc, hw, ec = _mix_shapes(xt, e)
    at, at_next = _alpha(at, B, xt.device), _alpha(at_next, B, xt.device)
    g_xt = torch.empty_like(xt)
    g_e = None if not want_g_e else (g_e_out if g_e_out is not None else torch.empty_like(e))
    if g_e is not None and g_e.shape != e.shape:
        raise _lib.NhmcError('g_e_out must have the shape of the score output')
    rc = lib.nhmc_ddim_mix_bwd(_p(gout, torch.float32, 'gout'), _p(gout2, torch.float32, 'gout2'),
                               _p(g_x0, torch.float32, 'g_x0'), _p(xt, torch.float32, 'xt'), _p(e, torch.float32, 'e'), ec, _p(at), _p(at_next),
                               int(final_clip), _p(g_xt), _p(g_e), int(g_e_out is None), B, Cc, hw, _stream())
    _lib.check(rc, 'nhmc_ddim_mix_bwd')
    return g_xt, g_e


def ddim_mix_bwd_inpaint(xt, e, at, at_next, y, slot, g_e_out=None, loss_out=None):
    """Last-step VJP fused with the inpainting data term -> (loss [B] float64, g_xt, g_e)."""
    dims, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, True)
    loss = _two_pass('nhmc_ddim_mix_bwd_inpaint', leapfrog_tiles(dims[1] * dims[2]), dims[0], xt.device, loss_out,
                     (*mix, _p(y, torch.float32, 'y'), _p(slot, torch.int32, 'slot'), y.shape[1], *grads), dims)
    return (loss, *outs)


def ddim_mix_bwd_inpaint_px(xt, e, at, at_next, y, mask_words, prefix, g_e_out=None, loss_out=None):
    """Whole-pixel-mask form of ddim_mix_bwd_inpaint: bit mask + prefix counts instead of the dense slot map."""
    (B, Cc, hw), mix, grads, (g_xt, g_e), alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, True)
    # _two_pass written out: the flagship's per-step wrapper, and at one chain per call the step is launch-bound
    lib = _lib.load()
    tiles = lib.nhmc_inpaint_px_tiles(Cc, hw)
    ws = torch.empty(B * tiles, dtype=torch.float64, device=xt.device)
    rc = lib.nhmc_ddim_mix_bwd_inpaint_px(*mix, _p(y, torch.float32, 'y'), _p(mask_words, torch.int32, 'mask_words'),
                                          _p(prefix, torch.int32, 'prefix'), y.shape[1], *grads, _p(ws), B, Cc, hw, _stream())
    _lib.check(rc, 'nhmc_ddim_mix_bwd_inpaint_px')
    return sum_partials(ws, tiles, B, out=loss_out), g_xt, g_e


def _square(xt):
    if xt.shape[3] != xt.shape[2]:
        raise _lib.NhmcError('square images only')
    return xt.shape[0], xt.shape[1], xt.shape[2]


def ddim_mix_bwd_sr(xt, e, at, at_next, y, ratio, g_e_out=None, loss_out=None):
    """Last-step VJP fused with the super-resolution data term -> (loss [B] float64, g_xt, g_e)."""
    B, Cc, dim = _square(xt)
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, False)
    loss = _two_pass('nhmc_ddim_mix_bwd_sr', _lib.load().nhmc_sr_vjp_tiles(Cc, dim, ratio), B, xt.device, loss_out,
                     (*mix, _p(y, torch.float32, 'y'), ratio, *grads), (B, Cc, dim))
    return (loss, *outs)


# ---- a12-a15 --------------------------------------------------------------------------------
NO_LOSS = object()      # pass as loss_out: the per-chain loss is not wanted (a MID leapfrog step uses only the gradient)


def _two_pass(entry, tiles, n_chains, device, loss_out, before, after):
    """The two-pass loss every data-term entry shares: `entry(*before, partials, *after, stream)` leaves `tiles` float64
    partials per chain, which sum_partials adds into loss_out -> the loss [n_chains] (None under NO_LOSS).  The caller
    holds the tensors behind the pointers in `before` / `after` until this returns."""
    ws = torch.empty(n_chains * tiles, dtype=torch.float64, device=device)
    _lib.check(getattr(_lib.load(), entry)(*before, _p(ws), *after, _stream()), entry)
    return sum_partials(ws, tiles, n_chains, out=loss_out)


def sum_partials(ws, tiles, n_chains, stride=1, offset=0, out=None):
    """Second pass of the two-pass loss: the tile partials of each chain added in a fixed order.  out=NO_LOSS skips the
    launch and returns None -- the sampler reads the loss of a trajectory's first and last evaluation only
    (main_sampling.py:697,717), so the L - 1 evaluations in between need the gradient alone."""
    if out is NO_LOSS:
        return None
    lib = _lib.load()
    if out is None:
        out = torch.empty(n_chains, dtype=torch.float64, device=ws.device)
    elif out.numel() != n_chains or out.dtype != torch.float64:
        raise _lib.NhmcError('sum_partials: out must be float64 of length n_chains')
    _lib.check(lib.nhmc_sum_partials(_p(ws, torch.float64), tiles, stride, offset, n_chains, _p(out), _stream()),
               'nhmc_sum_partials')
    return out


def data_inpaint(xt, y, slot, apply_clip=True, loss_out=None):
    """-> (loss [B] float64, g_xt).  slot: int32 [N] CHW map into y (-1 = masked)."""
    B, N = _chains_elems(xt)
    M = y.shape[1]
    if slot.numel() != N or y.shape[0] != B:
        raise _lib.NhmcError('slot / y shape mismatch')
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_inpaint', _lib.load().nhmc_data_tiles(N), B, xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), _p(y, torch.float32, 'y'), _p(slot, torch.int32, 'slot'), int(apply_clip), _p(g)),
                     (B, N, M))
    return loss, g


def inpaint_H(x, kept_chw):
    lib = _lib.load()
    B, N = _chains_elems(x)
    M = kept_chw.numel()
    y = torch.empty(B, M, dtype=torch.float32, device=x.device)
    _lib.check(lib.nhmc_inpaint_H(_p(x, torch.float32, 'x'), _p(kept_chw, torch.int32), _p(y), B, N, M, _stream()),
               'nhmc_inpaint_H')
    return y


def inpaint_Ht(y, slot, n_elem):
    lib = _lib.load()
    B, M = y.shape
    x = torch.empty(B, n_elem, dtype=torch.float32, device=y.device)
    _lib.check(lib.nhmc_inpaint_Ht(_p(y, torch.float32, 'y'), _p(slot, torch.int32), _p(x), B, n_elem, M, _stream()),
               'nhmc_inpaint_Ht')
    return x


def data_sr(xt, y, ratio, apply_clip=True, loss_out=None):
    B, Cc, dim = _square(xt)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_sr', _lib.load().nhmc_sr_tiles(Cc, dim, ratio), B, xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), _p(y, torch.float32, 'y'), ratio, int(apply_clip), _p(g)), (B, Cc, dim))
    return loss, g


def sr_H(x, ratio):
    lib = _lib.load()
    B, Cc, dim = x.shape[0], x.shape[1], x.shape[2]
    y = torch.empty(B, Cc * (dim // ratio) ** 2, dtype=torch.float32, device=x.device)
    _lib.check(lib.nhmc_sr_H(_p(x, torch.float32, 'x'), _p(y), ratio, B, Cc, dim, _stream()), 'nhmc_sr_H')
    return y


def sr_Ht(y, ratio, channels, dim, scale):
    lib = _lib.load()
    B = y.shape[0]
    x = torch.empty(B, channels * dim * dim, dtype=torch.float32, device=y.device)
    _lib.check(lib.nhmc_sr_Ht(_p(y, torch.float32, 'y'), _p(x), ratio, float(scale), B, channels, dim, _stream()),
               'nhmc_sr_Ht')
    return x


def _host_w(w, channels):
    """[V[0,0] .. V[C-1,0], s, U[0,0]]: the kernels read channels + 2 host floats (ABI 2; ABI 1 took `channels`)."""
    if len(w) != channels + 2:
        raise _lib.NhmcError(f'colorization weights: channels + 2 = {channels + 2} values (V[:,0], s, U[0,0]), got {len(w)}')
    arr = (C.c_float * len(w))(*[float(v) for v in w])
    return C.cast(arr, C.c_void_p), arr


def data_color(xt, y, w, apply_clip=True, loss_out=None):
    """w: host sequence [V[0,0] .. V[C-1,0], s, U[0,0]] of the grey row's SVD -> (loss [B] float64, g_xt)"""
    B, Cc, hw = xt.shape[0], xt.shape[1], xt[0, 0].numel()
    g = torch.empty_like(xt)
    wp, keep = _host_w(w, Cc)
    loss = _two_pass('nhmc_data_color', _lib.load().nhmc_color_tiles(hw), B, xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), _p(y, torch.float32, 'y'), wp, int(apply_clip), _p(g)), (B, Cc, hw))
    return loss, g


def ddim_mix_bwd_color(xt, e, at, at_next, y, w, g_e_out=None, loss_out=None):
    """Last-step VJP fused with the colorization data term -> (loss [B] float64, g_xt, g_e)."""
    dims, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, False)
    wp, keep = _host_w(w, dims[1])
    loss = _two_pass('nhmc_ddim_mix_bwd_color', _lib.load().nhmc_color_tiles(dims[2]), dims[0], xt.device, loss_out,
                     (*mix, _p(y, torch.float32, 'y'), wp, *grads), dims)
    return (loss, *outs)


def color_H(x, w):
    lib = _lib.load()
    B, Cc, hw = x.shape[0], x.shape[1], x[0, 0].numel()
    y = torch.empty(B, hw, dtype=torch.float32, device=x.device)
    wp, keep = _host_w(w, Cc)
    _lib.check(lib.nhmc_color_H(_p(x, torch.float32, 'x'), wp, _p(y), B, Cc, hw, _stream()), 'nhmc_color_H')
    return y


def color_Ht(y, w, channels, pinv=False):
    lib = _lib.load()
    B, hw = y.shape
    x = torch.empty(B, channels * hw, dtype=torch.float32, device=y.device)
    wp, keep = _host_w(w, channels)
    _lib.check(lib.nhmc_color_Ht(_p(y, torch.float32, 'y'), wp, int(pinv), _p(x), B, channels, hw, _stream()), 'nhmc_color_Ht')
    return x


def cs_H(x, kslot, m):
    lib = _lib.load()
    B, Cc, dim = x.shape[0], x.shape[1], x.shape[2]
    y = torch.zeros(B, m, dtype=torch.float32, device=x.device)
    tmp = torch.empty_like(x)
    _lib.check(lib.nhmc_cs_H(_p(x, torch.float32, 'x'), _p(kslot, torch.int32), _p(y), _p(tmp), B, Cc, dim, m, _stream()),
               'nhmc_cs_H')
    return y


def cs_Ht(y, kslot, channels, dim):
    lib = _lib.load()
    B, m = y.shape
    x = torch.empty(B, channels, dim, dim, dtype=torch.float32, device=y.device)
    tmp = torch.empty_like(x)
    _lib.check(lib.nhmc_cs_Ht(_p(y, torch.float32, 'y'), _p(kslot, torch.int32), _p(x), _p(tmp), B, channels, dim, m,
                              _stream()), 'nhmc_cs_Ht')
    return x.reshape(B, -1)


def _cs_io(xt, y_spec):
    """What data_cs and data_cs_vjp share -> (B, C, dim, tiles, tmp) after the shape check."""
    B, Cc, dim = xt.shape[0], xt.shape[1], xt.shape[2]
    if y_spec.numel() != xt.numel():
        raise _lib.NhmcError('data_cs: y_spec must have one entry per image element (spectrum layout)')
    tmp = torch.empty((1 if dim == 256 else 2,) + tuple(xt.shape), dtype=torch.float32, device=xt.device)
    return B, Cc, dim, _lib.load().nhmc_cs_tiles(Cc, dim), tmp


def data_cs(xt, y_spec, apply_clip=True, loss_out=None):
    """y_spec: the observation in spectrum layout [B, C, d, d], NaN where not observed (nhmc.h, nhmc_data_cs)."""
    B, Cc, dim, tiles, tmp = _cs_io(xt, y_spec)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_cs', tiles, B, xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), _p(y_spec, torch.float32, 'y_spec'), int(apply_clip), _p(g)),
                     (_p(tmp), B, Cc, dim))
    return loss, g


def data_cs_vjp(xt_next, y_spec, xt, e, at, at_next, g_e_out=None, loss_out=None):
    """Walsh-Hadamard CS data term on the clipped decode + VJP of the last DDIM step in the last row pass
    -> (loss [B] float64, g_xt, g_e).  y_spec: as in data_cs."""
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, False)
    B, Cc, dim, tiles, tmp = _cs_io(xt, y_spec)
    loss = _two_pass('nhmc_data_cs_vjp', tiles, B, xt.device, loss_out,
                     (_p(xt_next, torch.float32, 'xt_next'), _p(y_spec, torch.float32, 'y_spec'), *mix, *grads),
                     (_p(tmp), B, Cc, dim))
    return (loss, *outs)


def spectral_apply(x, L, R, Dmap, LoT, RoT):
    """out_c = Lo (D_c o (L^T X_c R)) Ro^T ; x: [B,C,d,d]"""
    lib = _lib.load()
    B, Cc, dim = x.shape[0], x.shape[1], x.shape[2]
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    rc = lib.nhmc_spectral_apply(_p(x, torch.float32, 'x'), _p(L, torch.float32), _p(R, torch.float32),
                                 _p(Dmap, torch.float32), _p(LoT, torch.float32), _p(RoT, torch.float32), _p(out),
                                 _p(tmp), B, Cc, dim, _stream())
    _lib.check(rc, 'nhmc_spectral_apply')
    return out


def sandwich_rect(x, S1, S2, mul=None):
    """x: [n_img, K1, R1]; t = x^T S1; out = (t^T S2) o mul -> [n_img, C1, C2] = (S1^T x S2) o mul  (mul [C1, C2] or None)"""
    lib = _lib.load()
    n, K1, R1 = x.shape
    C1, C2 = S1.shape[1], S2.shape[1]
    if S1.shape[0] != K1 or S2.shape[0] != R1:
        raise _lib.NhmcError('sandwich_rect: factor shapes do not chain')
    if mul is not None and tuple(mul.shape) != (C1, C2):
        raise _lib.NhmcError('sandwich_rect: the multiplier map must be [C1, C2]')
    out = torch.empty(n, C1, C2, dtype=torch.float32, device=x.device)
    tmp = torch.empty(n, R1, C1, dtype=torch.float32, device=x.device)
    rc = lib.nhmc_sandwich_rect(_p(x, torch.float32, 'x'), _p(S1, torch.float32), _p(S2, torch.float32), _p(mul, torch.float32, 'mul'),
                                _p(out), _p(tmp), n, K1, R1, C1, C2, _stream())
    _lib.check(rc, 'nhmc_sandwich_rect')
    return out


def _srconv_io(xt, f):
    """What data_srconv and data_srconv_vjp share: f = (V1 [d, sd], V1T [sd, d], U [sd, sd], UT [sd, sd], S [sd, sd])
    -> (the five factor pointers, tiles, tmp, the trailing (B, C, dim, sd)) after a shape check"""
    B, Cc, dim = xt.shape[0], xt.shape[1], xt.shape[2]
    V1, V1T, U, UT, S = f
    sd = U.shape[0]
    if tuple(V1.shape) != (dim, sd) or tuple(V1T.shape) != (sd, dim) or tuple(U.shape) != (sd, sd) or \
            tuple(UT.shape) != (sd, sd) or tuple(S.shape) != (sd, sd):
        raise _lib.NhmcError('SRConv factors: V1 [d, sd], V1^T [sd, d], U, U^T, S [sd, sd]')
    tmp = torch.empty(B * Cc * (dim * sd + 3 * sd * sd), dtype=torch.float32, device=xt.device)
    return [_p(t, torch.float32) for t in f], _lib.load().nhmc_srconv_tiles(Cc, sd), tmp, (B, Cc, dim, sd)


def data_srconv(xt, y, factors, apply_clip=True, loss_out=None):
    """factors: (V1, V1T, U, UT, S) as nhmc.operators.SRConv keeps them -> (loss [B] float64, g_xt)"""
    fac, tiles, tmp, dims = _srconv_io(xt, factors)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_srconv', tiles, dims[0], xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), _p(y, torch.float32, 'y'), *fac, int(apply_clip), _p(g)), (_p(tmp), *dims))
    return loss, g


def data_srconv_vjp(xt_next, y, factors, xt, e, at, at_next, g_e_out=None, loss_out=None):
    """Bicubic / strided-convolution data term on the clipped decode + VJP of the last DDIM step in the last product's
    epilogue -> (loss [B] float64, g_xt, g_e)."""
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, False)
    fac, tiles, tmp, dims = _srconv_io(xt, factors)
    loss = _two_pass('nhmc_data_srconv_vjp', tiles, dims[0], xt.device, loss_out,
                     (_p(xt_next, torch.float32, 'xt_next'), _p(y, torch.float32, 'y'), *fac, *mix, *grads),
                     (_p(tmp), *dims))
    return (loss, *outs)


def spectral_project(y, L, R):
    """y^ = L^T Y R per channel image (L = U1, R = U2): the observation in the operator's left singular basis."""
    lib = _lib.load()
    B, Cc, dim = y.shape[0], y.shape[1], y.shape[2]
    out, tmp = torch.empty_like(y), torch.empty_like(y)
    rc = lib.nhmc_spectral_project(_p(y, torch.float32, 'y'), _p(L, torch.float32), _p(R, torch.float32), _p(out), _p(tmp),
                                   B, Cc, dim, _stream())
    _lib.check(rc, 'nhmc_spectral_project')
    return out


def data_spectral(xt, y, factors, Dmap, apply_clip=True, loss_out=None, projected=False, DmapT=None):
    """factors: packed [8,d,d] = U1,U2,V1,V2,U1^T,U2^T,V1^T,V2^T -> (loss [B] float64, g_xt).
    Eight-product (reference-order) form: `y` is the observation with every channel plane TRANSPOSED and DmapT the
    multiplier map likewise (nhmc.h, nhmc_data_spectral).  projected: `y` is spectral_project(y, U1, U2) (natural
    orientation) and the four-product form runs."""
    entry, ops, tiles, tmp, dims = _spectral_io(xt, y, factors, Dmap, DmapT, projected)
    g = torch.empty_like(xt)
    loss = _two_pass(entry, tiles, dims[0], xt.device, loss_out, (_p(xt, torch.float32, 'xt'), *ops, int(apply_clip), _p(g)),
                     (_p(tmp), *dims))
    return loss, g


def _spectral_io(xt, y, factors, Dmap, DmapT, projected):
    """What data_spectral and data_spectral_vjp share, and the one place that chooses between the two forms
    -> (entry of the data term (the VJP form's is entry + '_vjp'), the operands after the image: y, factors and the
    form's multiplier maps, tiles, tmp, the trailing (B, C, dim))"""
    B, Cc, dim = xt.shape[0], xt.shape[1], xt.shape[2]
    ops = (_p(y, torch.float32, 'y' if projected else 'yT'), _p(factors, torch.float32, 'factors'), _p(Dmap, torch.float32, 'Dmap'))
    if not projected:
        if DmapT is None:
            raise _lib.NhmcError('data_spectral: the eight-product form needs DmapT (Dmap with every plane transposed)')
        ops += (_p(DmapT, torch.float32, 'DmapT'),)
    tmp = torch.empty((1 if projected else 2,) + tuple(xt.shape), dtype=torch.float32, device=xt.device)
    entry = 'nhmc_data_spectral_proj' if projected else 'nhmc_data_spectral'
    return entry, ops, _lib.load().nhmc_spectral_tiles(Cc, dim), tmp, (B, Cc, dim)


def data_spectral_vjp(xt_next, y, factors, Dmap, xt, e, at, at_next, g_e_out=None, loss_out=None, projected=False, DmapT=None):
    """Spectral data term on the clipped decode `xt_next` + VJP of the last DDIM step (inputs xt, e) in the last
    product's epilogue -> (loss [B] float64, g_xt, g_e).  y / DmapT / projected: as in data_spectral."""
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, False)
    entry, ops, tiles, tmp, dims = _spectral_io(xt, y, factors, Dmap, DmapT, projected)
    loss = _two_pass(entry + '_vjp', tiles, dims[0], xt.device, loss_out,
                     (_p(xt_next, torch.float32, 'xt_next'), *ops, *mix, *grads), (_p(tmp), *dims))
    return (loss, *outs)


# ---- nonlinear operators: HDR, phase retrieval -------------------------------------------------
def hdr_H(x):
    """clip(x / 0.5, -1, 1) elementwise, same shape."""
    lib = _lib.load()
    out = torch.empty_like(x)
    _lib.check(lib.nhmc_hdr_H(_p(x, torch.float32, 'x'), _p(out), x.numel(), _stream()), 'nhmc_hdr_H')
    return out


def _dense_y(y, xt):
    B, N = _chains_elems(xt)
    if y.shape[0] != B or y[0].numel() != N:
        raise _lib.NhmcError(f'the observation must have one entry per image element ({tuple(y.shape)} vs {tuple(xt.shape)})')
    return B, N


def data_hdr(xt, y, apply_clip=True, loss_out=None):
    """-> (loss [B] float64, g_xt) for H = clip(2 x); y dense, one entry per image element."""
    B, N = _dense_y(y, xt)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_hdr', _lib.load().nhmc_data_tiles(N), B, xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), _p(y, torch.float32, 'y'), int(apply_clip), _p(g)), (B, N))
    return loss, g


def mix_bwd_hdr(xt, e, at, at_next, y, g_e_out=None, loss_out=None):
    """Last-step VJP fused with the HDR data term -> (loss [B] float64, g_xt, g_e)."""
    dims, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, True)
    _dense_y(y, xt)
    loss = _two_pass('nhmc_mix_bwd_hdr', leapfrog_tiles(dims[1] * dims[2]), dims[0], xt.device, loss_out,
                     (*mix, _p(y, torch.float32, 'y'), *grads), dims)
    return (loss, *outs)


def _phase_shapes(x, fac, pad, side=None):
    """x: [B, C, s, s] (s = dim, or n = dim + 2 pad when side == 'n') -> B, C, dim, n after checking the packed factors."""
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise _lib.NhmcError(f'phase retrieval takes [B, C, s, s] planes, got {tuple(x.shape)}')
    B, Cc, s = x.shape[0], x.shape[1], x.shape[2]
    dim = s - 2 * pad if side == 'n' else s
    n = dim + 2 * pad
    if dim <= 0 or dim % 32 or (2 * pad) % 32:
        raise _lib.NhmcError('phase retrieval needs img_dim % 32 == 0 and (2 pad) % 32 == 0')
    if fac.numel() != 6 * n * dim:
        raise _lib.NhmcError(f'phase factors: expected {6 * n * dim} floats for dim {dim}, pad {pad}, got {fac.numel()}')
    return B, Cc, dim, n


def _phase_tmp(B, Cc, dim, pad, device):
    return torch.empty(_lib.load().nhmc_phase_tmp_floats(B, Cc, dim, pad), dtype=torch.float32, device=device)


def phase_H(x, fac, pad, spectrum=False):
    """|fft2c(pad(x))| -> [B, C, n, n]; spectrum=True: [Re ; Im] -> [B, C, 2, n, n]."""
    lib = _lib.load()
    B, Cc, dim, n = _phase_shapes(x, fac, pad)
    out = torch.empty((B, Cc, 2, n, n) if spectrum else (B, Cc, n, n), dtype=torch.float32, device=x.device)
    tmp = _phase_tmp(B, Cc, dim, pad, x.device)
    rc = lib.nhmc_phase_H(_p(x, torch.float32, 'x'), _p(fac, torch.float32, 'fac'), int(spectrum), _p(out), _p(tmp), B, Cc, dim, pad,
                          _stream())
    _lib.check(rc, 'nhmc_phase_H')
    return out


def phase_pinv(y, fac, pad):
    """crop(|ifft2c(y)|): y [B, C, n, n] -> [B, C, dim, dim]."""
    lib = _lib.load()
    B, Cc, dim, n = _phase_shapes(y, fac, pad, side='n')
    out = torch.empty(B, Cc, dim, dim, dtype=torch.float32, device=y.device)
    tmp = _phase_tmp(B, Cc, dim, pad, y.device)
    rc = lib.nhmc_phase_pinv(_p(y, torch.float32, 'y'), _p(fac, torch.float32, 'fac'), _p(out), _p(tmp), B, Cc, dim, pad, _stream())
    _lib.check(rc, 'nhmc_phase_pinv')
    return out


def phase_adjoint(w, fac, pad):
    """The adjoint of phase_H(spectrum=True): w [B, C, 2, n, n] -> [B, C, dim, dim]."""
    lib = _lib.load()
    if w.dim() != 5 or w.shape[2] != 2:
        raise _lib.NhmcError('phase_adjoint takes [B, C, 2, n, n]')
    B, Cc, dim, n = _phase_shapes(w[:, :, 0], fac, pad, side='n')
    out = torch.empty(B, Cc, dim, dim, dtype=torch.float32, device=w.device)
    tmp = _phase_tmp(B, Cc, dim, pad, w.device)
    rc = lib.nhmc_phase_adjoint(_p(w, torch.float32, 'w'), _p(fac, torch.float32, 'fac'), _p(out), _p(tmp), B, Cc, dim, pad, _stream())
    _lib.check(rc, 'nhmc_phase_adjoint')
    return out


def _phase_io(xt, y, fac, pad):
    """What data_phase and data_phase_vjp share -> (tiles, tmp, the trailing (B, C, dim, pad)) after the shape checks."""
    B, Cc, dim, n = _phase_shapes(xt, fac, pad)
    if tuple(y.shape) != (B, Cc, n, n):
        raise _lib.NhmcError(f'phase observation must be [{B}, {Cc}, {n}, {n}], got {tuple(y.shape)}')
    return _lib.load().nhmc_phase_tiles(Cc, dim, pad), _phase_tmp(B, Cc, dim, pad, xt.device), (B, Cc, dim, pad)


def _xt_next(xt_next, xt):
    """The checked pointer of the clipped decode handed to a VJP form."""
    if xt_next.shape != xt.shape:
        raise _lib.NhmcError('xt_next must have the shape of xt')
    return _p(xt_next, torch.float32, 'xt_next')


def data_phase(xt, y, fac, pad, apply_clip=True, loss_out=None):
    """-> (loss [B] float64, g_xt) for H = |fft2c(pad(x))|; y [B, C, n, n]."""
    tiles, tmp, dims = _phase_io(xt, y, fac, pad)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_phase', tiles, dims[0], xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), _p(y, torch.float32, 'y'), _p(fac, torch.float32, 'fac'), int(apply_clip), _p(g)),
                     (_p(tmp), *dims))
    return loss, g


def data_phase_vjp(xt_next, y, fac, pad, xt, e, at, at_next, g_e_out=None, loss_out=None):
    """Phase-retrieval data term on the clipped decode `xt_next` + VJP of the last DDIM step (inputs xt, e) in the last
    product's epilogue -> (loss [B] float64, g_xt, g_e)."""
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, False)
    tiles, tmp, dims = _phase_io(xt, y, fac, pad)
    loss = _two_pass('nhmc_data_phase_vjp', tiles, dims[0], xt.device, loss_out,
                     (_xt_next(xt_next, xt), _p(y, torch.float32, 'y'), _p(fac, torch.float32, 'fac'), *mix, *grads),
                     (_p(tmp), *dims))
    return (loss, *outs)


# ---- Fourier sampling (mri<R>, fourier): the weighted spectrum at pad = 0 ------------------------------
def _fourier_shapes(x, fac, w):
    """x: [B, C, d, d]; fac: the phase factors at pad = 0; w: the weight map [d, d] -> B, C, d."""
    B, Cc, dim, _ = _phase_shapes(x, fac, 0)
    if tuple(w.shape) != (dim, dim):
        raise _lib.NhmcError(f'the k-space weights must be [{dim}, {dim}], got {tuple(w.shape)}')
    return B, Cc, dim


def _fourier_io(xt, y, fac, w):
    """What data_fourier and data_fourier_vjp share -> (tiles, tmp, operands (y, fac, w), the trailing (B, C, dim))."""
    B, Cc, dim = _fourier_shapes(xt, fac, w)
    if tuple(y.shape) != (B, Cc, 2, dim, dim):
        raise _lib.NhmcError(f'the k-space observation must be [{B}, {Cc}, 2, {dim}, {dim}], got {tuple(y.shape)}')
    ops = (_p(y, torch.float32, 'y'), _p(fac, torch.float32, 'fac'), _p(w, torch.float32, 'w'))
    return _lib.load().nhmc_phase_tiles(Cc, dim, 0), _phase_tmp(B, Cc, dim, 0, xt.device), ops, (B, Cc, dim)


def fourier_H(x, fac, w):
    """[w o Re Y ; w o Im Y] of the centred orthonormal 2-D DFT of every plane: [B, C, d, d] -> [B, C, 2, d, d]."""
    lib = _lib.load()
    B, Cc, dim = _fourier_shapes(x, fac, w)
    out = torch.empty(B, Cc, 2, dim, dim, dtype=torch.float32, device=x.device)
    tmp = _phase_tmp(B, Cc, dim, 0, x.device)
    rc = lib.nhmc_fourier_H(_p(x, torch.float32, 'x'), _p(fac, torch.float32, 'fac'), _p(w, torch.float32, 'w'), _p(out), _p(tmp),
                            B, Cc, dim, _stream())
    _lib.check(rc, 'nhmc_fourier_H')
    return out


def data_fourier(xt, y, fac, w, apply_clip=True, loss_out=None):
    """-> (loss [B] float64, g_xt) for H = w o fft2c(x); y [B, C, 2, d, d], read only where w > 0."""
    tiles, tmp, ops, dims = _fourier_io(xt, y, fac, w)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_fourier', tiles, dims[0], xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), *ops, int(apply_clip), _p(g)), (_p(tmp), *dims))
    return loss, g


def data_fourier_vjp(xt_next, y, fac, w, xt, e, at, at_next, g_e_out=None, loss_out=None):
    """Fourier-sampling data term on the clipped decode `xt_next` + VJP of the last DDIM step (inputs xt, e) in the last
    product's epilogue -> (loss [B] float64, g_xt, g_e)."""
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, False)
    tiles, tmp, ops, dims = _fourier_io(xt, y, fac, w)
    loss = _two_pass('nhmc_data_fourier_vjp', tiles, dims[0], xt.device, loss_out,
                     (_xt_next(xt_next, xt), *ops, *mix, *grads), (_p(tmp), *dims))
    return (loss, *outs)


# ---- modulated Fourier operators (mcmri<R>, cdp<K>): the spectrum of the image times K complex maps --------
def _modfourier_shapes(x, maps, fac, w):
    """x: [B, C, d, d]; maps: [K, 2, d, d] (a real and an imaginary plane per map); fac: the phase factors at pad = 0;
    w: the weight map [d, d] -> B, C, K, d."""
    B, Cc, dim, _ = _phase_shapes(x, fac, 0)
    if maps.dim() != 4 or tuple(maps.shape[1:]) != (2, dim, dim) or not 1 <= maps.shape[0] <= 32:
        raise _lib.NhmcError(f'the modulation maps must be [K, 2, {dim}, {dim}] with 1 <= K <= 32, got {tuple(maps.shape)}')
    if tuple(w.shape) != (dim, dim):
        raise _lib.NhmcError(f'the k-space weights must be [{dim}, {dim}], got {tuple(w.shape)}')
    if B * Cc * 2 * maps.shape[0] > 65535:
        raise _lib.NhmcError(f'{B} chains x {Cc} channels x {maps.shape[0]} maps are {B * Cc * 2 * maps.shape[0]} modulated '
                             f'planes, the spectral chain takes 65535 per call')
    return B, Cc, maps.shape[0], dim


def _modfourier_tmp(B, Cc, Km, dim, device):
    return torch.empty(_lib.load().nhmc_modfourier_tmp_floats(B, Cc, Km, dim), dtype=torch.float32, device=device)


def _modfourier_obs_shape(B, Cc, Km, dim, modulus):
    return (B, Cc, Km, dim, dim) if modulus else (B, Cc, Km, 2, dim, dim)


def _modfourier_io(xt, y, maps, fac, w, modulus):
    """What data_modfourier and data_modfourier_vjp share -> (tiles, tmp, operands (y, maps, fac, w, modulus), the trailing
    (B, C, K, dim))."""
    B, Cc, Km, dim = _modfourier_shapes(xt, maps, fac, w)
    want = _modfourier_obs_shape(B, Cc, Km, dim, modulus)
    if tuple(y.shape) != want:
        raise _lib.NhmcError(f'the observation must be {list(want)}, got {tuple(y.shape)}')
    ops = (_p(y, torch.float32, 'y'), _p(maps, torch.float32, 'maps'), _p(fac, torch.float32, 'fac'), _p(w, torch.float32, 'w'),
           int(bool(modulus)))
    return (_lib.load().nhmc_modfourier_tiles(Cc, Km, dim), _modfourier_tmp(B, Cc, Km, dim, xt.device), ops, (B, Cc, Km, dim))


def modfourier_H(x, maps, fac, w, modulus=False):
    """The centred orthonormal 2-D DFT of every plane times every map, weighted: [B, C, d, d] -> [w o Re Y ; w o Im Y]
    [B, C, K, 2, d, d], or under `modulus` w o |Y| [B, C, K, d, d]."""
    lib = _lib.load()
    B, Cc, Km, dim = _modfourier_shapes(x, maps, fac, w)
    out = torch.empty(_modfourier_obs_shape(B, Cc, Km, dim, modulus), dtype=torch.float32, device=x.device)
    tmp = _modfourier_tmp(B, Cc, Km, dim, x.device)
    rc = lib.nhmc_modfourier_H(_p(x, torch.float32, 'x'), _p(maps, torch.float32, 'maps'), _p(fac, torch.float32, 'fac'),
                               _p(w, torch.float32, 'w'), int(bool(modulus)), _p(out), _p(tmp), B, Cc, Km, dim, _stream())
    _lib.check(rc, 'nhmc_modfourier_H')
    return out


def modfourier_Ht(v, maps, fac, w):
    """The exact adjoint of the linear modfourier_H: v [B, C, K, 2, d, d] -> [B, C, d, d]."""
    lib = _lib.load()
    if v.dim() != 6 or v.shape[3] != 2:
        raise _lib.NhmcError(f'modfourier_Ht takes [B, C, K, 2, d, d], got {tuple(v.shape)}')
    B, Cc, Km, dim = _modfourier_shapes(v[:, :, 0, 0], maps, fac, w)
    if v.shape[2] != Km:
        raise _lib.NhmcError(f'modfourier_Ht: v holds {v.shape[2]} maps, the operator {Km}')
    out = torch.empty(B, Cc, dim, dim, dtype=torch.float32, device=v.device)
    tmp = _modfourier_tmp(B, Cc, Km, dim, v.device)
    rc = lib.nhmc_modfourier_Ht(_p(v, torch.float32, 'v'), _p(maps, torch.float32, 'maps'), _p(fac, torch.float32, 'fac'),
                                _p(w, torch.float32, 'w'), _p(out), _p(tmp), B, Cc, Km, dim, _stream())
    _lib.check(rc, 'nhmc_modfourier_Ht')
    return out


def data_modfourier(xt, y, maps, fac, w, modulus=False, apply_clip=True, loss_out=None):
    """-> (loss [B] float64, g_xt) for the modulated Fourier operator; y as modfourier_H returns it, read only where w > 0."""
    tiles, tmp, ops, dims = _modfourier_io(xt, y, maps, fac, w, modulus)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_modfourier', tiles, dims[0], xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), *ops, int(apply_clip), _p(g)), (_p(tmp), *dims))
    return loss, g


def data_modfourier_vjp(xt_next, y, maps, fac, w, modulus, xt, e, at, at_next, g_e_out=None, loss_out=None):
    """The modulated Fourier data term on the clipped decode `xt_next` + VJP of the last DDIM step (inputs xt, e) in the
    demodulating kernel's epilogue -> (loss [B] float64, g_xt, g_e)."""
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, False)
    tiles, tmp, ops, dims = _modfourier_io(xt, y, maps, fac, w, modulus)
    loss = _two_pass('nhmc_data_modfourier_vjp', tiles, dims[0], xt.device, loss_out,
                     (_xt_next(xt_next, xt), *ops, *mix, *grads), (_p(tmp), *dims))
    return (loss, *outs)


# ---- general 2-D PSF blur (deblur_motion) --------------------------------------------------------
class BlurTaps:
    """The compacted tap list of a 2-D PSF (include/nhmc.h): the non-zero entries of k [K, K] in row-major order as
    (dy, dx) = (i - R, j - R) and w.  `off` int32 [T, 2] and `w` float32 [T] are the host copies, `off_dev` / `w_dev` what
    the kernels read.  Built and checked once (nhmc_blur2d_check_taps); constructible on 'cpu' (no device copies used)."""

    def __init__(self, kernel2d, device):
        k = torch.as_tensor(kernel2d).detach().cpu()
        if k.dim() != 2 or k.shape[0] != k.shape[1]:
            raise _lib.NhmcError(f'a PSF is a square [K, K] array, got {tuple(k.shape)}')
        k = k.to(torch.float32).contiguous()
        self.ksize = K_ = int(k.shape[0])
        if K_ % 2 == 0 or K_ > 63:
            raise _lib.NhmcError(f'PSF size must be odd and at most 63, got {K_}')
        self.radius = R = (K_ - 1) // 2
        ij = torch.nonzero(k)                                       # row-major: i ascending, then j
        if ij.shape[0] == 0:
            raise _lib.NhmcError('the PSF has no non-zero entry')
        self.off = (ij - R).to(torch.int32).contiguous()
        self.w = k[ij[:, 0], ij[:, 1]].contiguous()
        self.n = int(ij.shape[0])
        rc = _lib.load().nhmc_blur2d_check_taps(C.c_void_p(self.off.data_ptr()), self.n, K_)
        _lib.check(rc, 'nhmc_blur2d_check_taps')
        self.off_dev, self.w_dev = self.off.to(device), self.w.to(device)
        # the halo the kernels stage is (ksize - 1) / 2: hand them the list's own extent, not the array's (a camera-shake
        # path seldom fills its 61 x 61 support, and a rim of zeros then costs nothing)
        self.extent = 2 * int(self.off.abs().max()) + 1

    def args(self):
        return _p(self.off_dev, torch.int32, 'taps_off'), _p(self.w_dev, torch.float32, 'taps_w'), self.n, self.extent


def _blur_shapes(x):
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise _lib.NhmcError(f'the 2-D blur takes [B, C, d, d] planes, got {tuple(x.shape)}')
    return x.shape[0], x.shape[1], x.shape[2]


def blur2d_tiles(channels, dim):
    return _lib.load().nhmc_blur2d_tiles(channels, dim)


def blur2d_apply(x, taps, transpose=False):
    """H x (correlation with the PSF, zero boundary), or the exact adjoint H^T x -> same shape."""
    lib = _lib.load()
    B, Cc, dim = _blur_shapes(x)
    out = torch.empty_like(x)
    rc = lib.nhmc_blur2d_apply(_p(x, torch.float32, 'x'), *taps.args(), int(transpose), _p(out), B, Cc, dim, _stream())
    _lib.check(rc, 'nhmc_blur2d_apply')
    return out


def _blur_io(xt, y):
    """What data_blur2d and data_blur2d_vjp share -> (tiles, tmp, the trailing (B, C, dim)) after the shape checks."""
    dims = _blur_shapes(xt)
    if tuple(y.shape) != tuple(xt.shape):
        raise _lib.NhmcError(f'the blur observation has the image shape {tuple(xt.shape)}, got {tuple(y.shape)}')
    return _lib.load().nhmc_blur2d_tiles(dims[1], dims[2]), torch.empty_like(xt), dims


def data_blur2d(xt, y, taps, apply_clip=True, loss_out=None):
    """-> (loss [B] float64, g_xt) for H = the PSF blur; y [B, C, d, d]."""
    tiles, tmp, dims = _blur_io(xt, y)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_blur2d', tiles, dims[0], xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), _p(y, torch.float32, 'y'), *taps.args(), int(apply_clip), _p(g)),
                     (_p(tmp), *dims))
    return loss, g


def data_blur2d_vjp(xt_next, y, taps, xt, e, at, at_next, g_e_out=None, loss_out=None):
    """Blur data term on the clipped decode `xt_next` + VJP of the last DDIM step (inputs xt, e) in the adjoint pass's
    epilogue -> (loss [B] float64, g_xt, g_e)."""
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, True)
    tiles, tmp, dims = _blur_io(xt, y)
    loss = _two_pass('nhmc_data_blur2d_vjp', tiles, dims[0], xt.device, loss_out,
                     (_xt_next(xt_next, xt), _p(y, torch.float32, 'y'), *taps.args(), *mix, *grads), (_p(tmp), *dims))
    return (loss, *outs)


# ---- sparse linear operators (SparseLinear, ct<V>) -----------------------------------------------
def _is_scipy_like(a):
    return all(hasattr(a, k) for k in ('tocoo', 'shape')) and not isinstance(a, torch.Tensor)


def _coo_of(matrix, shape):
    """Any accepted matrix form -> (rows int64, cols int64, vals float64, (m, n)), host tensors, entries in any order."""
    if isinstance(matrix, torch.Tensor):
        a = matrix.detach().cpu()
        if a.dim() != 2:
            raise _lib.NhmcError(f'a sparse operator is a 2-D matrix, got {tuple(a.shape)}')
        if a.layout == torch.sparse_csr:
            crow, col, val = a.crow_indices().long(), a.col_indices().long(), a.values()
            row = torch.repeat_interleave(torch.arange(a.shape[0]), crow[1:] - crow[:-1])
        elif a.layout == torch.sparse_coo:
            idx = a._indices() if not a.is_coalesced() else a.indices()
            val = a._values() if not a.is_coalesced() else a.values()
            row, col = idx[0].long(), idx[1].long()
        else:
            raise _lib.NhmcError('a torch matrix must be sparse COO or sparse CSR (use .to_sparse())')
        return row, col, val.to(torch.float64), (int(a.shape[0]), int(a.shape[1]))
    if _is_scipy_like(matrix):                                   # duck-typed: scipy is not a dependency
        coo = matrix.tocoo()
        as_t = lambda v, dt: torch.as_tensor(v.astype(dt))
        return (as_t(coo.row, 'int64'), as_t(coo.col, 'int64'), as_t(coo.data, 'float64'),
                (int(coo.shape[0]), int(coo.shape[1])))
    if isinstance(matrix, (tuple, list)) and len(matrix) == 3:
        if shape is None or len(shape) != 2:
            raise _lib.NhmcError('the (row_ptr, col, val) form needs shape=(m, n)')
        m, n = int(shape[0]), int(shape[1])
        rp, col, val = (torch.as_tensor(v).detach().cpu().reshape(-1) for v in matrix)
        rp, col = rp.long(), col.long()
        if m < 1:
            raise _lib.NhmcError(f'a sparse operator needs at least one row, got m = {m}')
        if rp.numel() != m + 1 or col.numel() != val.numel():
            raise _lib.NhmcError(f'(row_ptr, col, val): row_ptr has m + 1 = {m + 1} entries and col as many as val')
        cnt = rp[1:] - rp[:-1]
        if int(rp[0]) != 0 or int(rp[-1]) != col.numel() or bool((cnt < 0).any()):
            raise _lib.NhmcError('(row_ptr, col, val): row_ptr must start at 0, end at nnz and not decrease')
        row = torch.repeat_interleave(torch.arange(m), cnt)
        return row, col, val.to(torch.float64), (m, n)
    raise _lib.NhmcError('a sparse operator is a torch sparse COO / CSR tensor, a scipy.sparse matrix or a triple '
                         '(row_ptr, col, val) with shape=')


def _csr_lists(row, col, val, m):
    """Entries sorted by (row, col) -> (row_ptr int32 [m + 1], col int32, val float32)."""
    rp = torch.zeros(m + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(row, minlength=m), 0)
    return rp.to(torch.int32).contiguous(), col.to(torch.int32).contiguous(), val.contiguous()


class SparseMatrix:
    """The canonical CSR pair of a sparse operator (include/nhmc.h): A [m, n] and A^T, each as (row_ptr int32, col int32,
    val float32).  Entries sorted by (row, column), duplicates summed in float64 and rounded to fp32, an entry whose fp32
    value is 0 dropped; A^T by a stable transpose (within its rows the entries ascend by their row in A, same fp32 values).
    `row_ptr / col / val` and `t_row_ptr / t_col / t_val` are the host copies, `dev` / `t_dev` what the kernels read.  Built
    and checked once (nhmc_sparse_check on both lists); constructible on 'cpu' (no device copies used)."""

    def __init__(self, matrix, device, shape=None):
        row, col, val, (m, n) = _coo_of(matrix, shape)
        if m < 1 or n < 1:
            raise _lib.NhmcError(f'a sparse operator needs at least one row and one column, got {m} x {n}')
        if row.numel() and (int(row.min()) < 0 or int(row.max()) >= m):
            raise _lib.NhmcError(f'a row index lies outside [0, {m})')
        if col.numel() and (int(col.min()) < 0 or int(col.max()) >= n):
            raise _lib.NhmcError(f'a column index lies outside [0, {n})')
        key = row * n + col
        ukey, inv = torch.unique(key, return_inverse=True)                  # sorted by (row, col)
        order = torch.argsort(inv, stable=True)                             # duplicates are summed in input order
        sval = torch.zeros(ukey.numel(), dtype=torch.float64).index_add_(0, inv[order], val[order]).to(torch.float32)
        keep = sval != 0                                                    # a zero is not an entry (NaN != 0 stays)
        ukey, sval = ukey[keep], sval[keep]
        if ukey.numel() < 1:
            raise _lib.NhmcError('the sparse operator has no non-zero entry')
        if ukey.numel() >= 2 ** 31:
            raise _lib.NhmcError('the sparse operator has 2^31 entries or more')
        self.m, self.n, self.nnz = m, n, int(ukey.numel())
        r, c = torch.div(ukey, n, rounding_mode='floor'), ukey % n
        self.row_ptr, self.col, self.val = _csr_lists(r, c, sval, m)
        t_order = torch.argsort(c, stable=True)                             # stable: rows of A ascend within a row of A^T
        self.t_row_ptr, self.t_col, self.t_val = _csr_lists(c[t_order], r[t_order], sval[t_order], n)
        lib = _lib.load()
        for rp, cl, rows, cols in ((self.row_ptr, self.col, m, n), (self.t_row_ptr, self.t_col, n, m)):
            rc = lib.nhmc_sparse_check(C.c_void_p(rp.data_ptr()), C.c_void_p(cl.data_ptr()), rows, cols, self.nnz)
            _lib.check(rc, 'nhmc_sparse_check')
        self.dev = tuple(t.to(device) for t in (self.row_ptr, self.col, self.val))
        self.t_dev = tuple(t.to(device) for t in (self.t_row_ptr, self.t_col, self.t_val))

    @staticmethod
    def _ptrs(lists):
        return (_p(lists[0], torch.int32, 'row_ptr'), _p(lists[1], torch.int32, 'col'), _p(lists[2], torch.float32, 'val'))

    def args(self, transpose=False):
        """-> (row_ptr, col, val, rows, cols, nnz) of A, or of A^T."""
        if transpose:
            return (*self._ptrs(self.t_dev), self.n, self.m, self.nnz)
        return (*self._ptrs(self.dev), self.m, self.n, self.nnz)

    def both(self):
        """-> the six list pointers of the data terms: A, then A^T."""
        return (*self._ptrs(self.dev), *self._ptrs(self.t_dev))


def sparse_tiles(channels, m):
    return _lib.load().nhmc_sparse_tiles(channels, m)


def _sparse_planes(x, cols, what):
    if x.dim() != 3 or x.shape[2] != cols:
        raise _lib.NhmcError(f'{what} takes [B, C, {cols}] planes, got {tuple(x.shape)}')
    return x.shape[0], x.shape[1]


def sparse_apply(x, mat, transpose=False):
    """A x for x [B, C, n] -> [B, C, m], or the exact adjoint A^T x for x [B, C, m] -> [B, C, n]."""
    lib = _lib.load()
    rp, cl, vl, rows, cols, nnz = mat.args(transpose)
    B, Cc = _sparse_planes(x, cols, 'the sparse product')
    out = torch.empty(B, Cc, rows, dtype=torch.float32, device=x.device)
    tmp = torch.empty(lib.nhmc_sparse_tmp_floats(B, Cc, mat.m, mat.n), dtype=torch.float32, device=x.device)
    rc = lib.nhmc_sparse_apply(_p(x, torch.float32, 'x'), rp, cl, vl, rows, cols, nnz, _p(out), _p(tmp), B, Cc, _stream())
    _lib.check(rc, 'nhmc_sparse_apply')
    return out


def _sparse_io(xt, y, mat):
    """What data_sparse and data_sparse_vjp share -> (the operands after the image: y, both lists, m, nnz; tiles; tmp;
    the trailing (B, C, dim)) after the shape checks."""
    if xt.dim() != 4 or xt.shape[2] != xt.shape[3] or xt.shape[2] * xt.shape[3] != mat.n:
        raise _lib.NhmcError(f'the sparse operator takes [B, C, d, d] images with d * d = {mat.n}, got {tuple(xt.shape)}')
    B, Cc, dim = xt.shape[0], xt.shape[1], xt.shape[2]
    if tuple(y.shape) != (B, Cc, mat.m):
        raise _lib.NhmcError(f'the sparse observation has the shape {(B, Cc, mat.m)}, got {tuple(y.shape)}')
    lib = _lib.load()
    tmp = torch.empty(lib.nhmc_sparse_tmp_floats(B, Cc, mat.m, mat.n), dtype=torch.float32, device=xt.device)
    ops = (_p(y, torch.float32, 'y'), *mat.both(), mat.m, mat.nnz)
    return ops, lib.nhmc_sparse_tiles(Cc, mat.m), tmp, (B, Cc, dim)


def data_sparse(xt, y, mat, apply_clip=True, loss_out=None):
    """-> (loss [B] float64, g_xt) for the sparse operator `mat`; xt [B, C, d, d], y [B, C, m]."""
    ops, tiles, tmp, dims = _sparse_io(xt, y, mat)
    g = torch.empty_like(xt)
    loss = _two_pass('nhmc_data_sparse', tiles, dims[0], xt.device, loss_out,
                     (_p(xt, torch.float32, 'xt'), *ops, int(apply_clip), _p(g)), (_p(tmp), *dims))
    return loss, g


def data_sparse_vjp(xt_next, y, mat, xt, e, at, at_next, g_e_out=None, loss_out=None):
    """Sparse data term on the clipped decode `xt_next` + VJP of the last DDIM step (inputs xt, e) in the adjoint pass's
    epilogue -> (loss [B] float64, g_xt, g_e)."""
    _, mix, grads, outs, alphas = _last_vjp_io(xt, e, at, at_next, g_e_out, True)
    ops, tiles, tmp, dims = _sparse_io(xt, y, mat)
    loss = _two_pass('nhmc_data_sparse_vjp', tiles, dims[0], xt.device, loss_out,
                     (_xt_next(xt_next, xt), *ops, *mix, *grads), (_p(tmp), *dims))
    return (loss, *outs)


# ---- a5-a7 ----------------------------------------------------------------------------------
def hamiltonian(sums_ws, n_elem, loss, sigma_y, m_inv, want_terms=False, sel=None):
    """sel (int32 [B]): loss is then the gradient cache's loss_pair [2, B] and chain c uses loss[sel[c], c]."""
    lib = _lib.load()
    B = loss.numel() if sel is None else sel.numel()
    H = torch.empty(B, dtype=torch.float32, device=loss.device)
    terms = torch.empty(B, 3, dtype=torch.float64, device=loss.device) if want_terms else None
    sy = _f64(sigma_y, B, loss.device)
    if sel is None:
        rc = lib.nhmc_hamiltonian(_p(sums_ws, torch.float64), leapfrog_tiles(n_elem), _p(loss, torch.float64, 'loss'),
                                  _p(sy), float(m_inv), _p(H), _p(terms), B, _stream())
    else:
        lp, ls = _loss_pair(loss, B)
        rc = lib.nhmc_hamiltonian_cached(_p(sums_ws, torch.float64), leapfrog_tiles(n_elem), lp, _p(sel, torch.int32, 'sel'),
                                         ls, _p(sy), float(m_inv), _p(H), _p(terms), B, _stream())
    _lib.check(rc, 'nhmc_hamiltonian' if sel is None else 'nhmc_hamiltonian_cached')
    return (H, terms) if want_terms else H


def metropolis(H0, H1, u, active=None):
    lib = _lib.load()
    B = H0.numel()
    acc = torch.empty(B, dtype=torch.int32, device=H0.device)
    dH = torch.empty(B, dtype=torch.float32, device=H0.device)
    rc = lib.nhmc_metropolis(_p(H0, torch.float32), _p(H1, torch.float32), _p(u, torch.float32, 'u'),
                             _p(active, torch.int32), _p(acc), _p(dH), B, _stream())
    _lib.check(rc, 'nhmc_metropolis')
    return acc, dH


def schedule_begin(state, sigma_0, epochs, sampling):
    lib = _lib.load()
    B = state['epoch'].numel()
    rc = lib.nhmc_schedule_begin(_p(state['epoch'], torch.int32), _p(state['tau'], torch.float64),
                                 _p(state['eps'], torch.float64), _p(state['sigma_y'], torch.float64),
                                 _p(state['eps_eff'], torch.float64), _p(state['active'], torch.int32),
                                 float(sigma_0), epochs, sampling, B, _stream())
    _lib.check(rc, 'nhmc_schedule_begin')


def accept_commit(accept, epoch, x, x_prop, xt_prop, samples, epochs, sampling):
    lib = _lib.load()
    B, N = _chains_elems(x)
    rc = lib.nhmc_accept_commit(_p(accept, torch.int32), _p(epoch, torch.int32), _p(x, torch.float32, 'x'),
                                _p(x_prop, torch.float32, 'x_prop'), _p(xt_prop, torch.float32, 'xt_prop'),
                                _p(samples, torch.float32, 'samples'), epochs, sampling, B, N, _stream())
    _lib.check(rc, 'nhmc_accept_commit')


def schedule_end(accept, state):
    lib = _lib.load()
    B = accept.numel()
    rc = lib.nhmc_schedule_end(_p(accept, torch.int32), _p(state['active'], torch.int32),
                               _p(state['epoch'], torch.int32), _p(state['rejected'], torch.int32),
                               _p(state['tau'], torch.float64), _p(state['eps'], torch.float64),
                               _p(state.get('n_accept'), torch.int32), _p(state.get('n_reject'), torch.int32),
                               B, _stream())
    _lib.check(rc, 'nhmc_schedule_end')


def latent_commit(accept, st, final_phase, keep, x, x_prop, xt_last, xt_prop, samples):
    lib = _lib.load()
    B, N = _chains_elems(x)
    rc = lib.nhmc_latent_commit(_p(accept, torch.int32), _p(st['has_prev'], torch.int32), _p(st['count'], torch.int32),
                                int(final_phase), int(keep), _p(x, torch.float32, 'x'), _p(x_prop, torch.float32, 'x_prop'),
                                _p(xt_last, torch.float32, 'xt_last'), _p(xt_prop, torch.float32, 'xt_prop'),
                                _p(samples, torch.float32, 'samples'), B, N, _stream())
    _lib.check(rc, 'nhmc_latent_commit')


def schedule_end_latent(accept, st, sigma_y_on_accept, final_phase):
    lib = _lib.load()
    rc = lib.nhmc_schedule_end_latent(_p(accept, torch.int32), _p(st['rejected'], torch.int32), _p(st['tau'], torch.float64),
                                      _p(st['eps'], torch.float64), _p(st['sigma_y'], torch.float64),
                                      _p(st['count'], torch.int32), _p(st['has_prev'], torch.int32),
                                      _p(st.get('n_accept'), torch.int32), float(sigma_y_on_accept), int(final_phase),
                                      accept.numel(), _stream())
    _lib.check(rc, 'nhmc_schedule_end_latent')


def leapfrog_mass(mode, x, p, g, inv_m, eps, sigma_y, sums_ws=None, g2=None, z=None, std_m=None, welford_on=None,
                  mean=None, m2=None, l=0):
    lib = _lib.load()
    B, N = _chains_elems(x)
    ep, sy = _f64(eps, B, x.device), _f64(sigma_y, B, x.device)          # two live tensors (never alias a freed block)
    rc = lib.nhmc_leapfrog_mass(mode, _p(x, torch.float32, 'x'), _p(p, torch.float32, 'p'), _p(z, torch.float32, 'z'),
                                _p(g, torch.float32, 'g'), _p(g2, torch.float32, 'g2'), _p(inv_m, torch.float32, 'inv_m'),
                                _p(std_m, torch.float32, 'std_m'), _p(ep), _p(sy),
                                _p(welford_on, torch.int32), _p(mean, torch.float32), _p(m2, torch.float32), int(l), B, N,
                                _p(sums_ws, torch.float64), _stream())
    _lib.check(rc, 'nhmc_leapfrog_mass')


def mass_from_variance(m2, L, flags, inv_m, std_m, tables, ws=None):
    """tables: (std_table, inv_table) float32 [N] on the device, by rank (nhmc.schedule.mass_tables(N, device))."""
    lib = _lib.load()
    B, N = _chains_elems(m2)
    std_t, inv_t = tables
    if std_t.numel() != N or inv_t.numel() != N:
        raise _lib.NhmcError('mass tables must have one entry per element (rank)')
    need = lib.nhmc_mass_sort_ws_bytes(B, N)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=m2.device)
    rc = lib.nhmc_mass_from_variance(_p(m2, torch.float32, 'm2'), int(L), _p(flags, torch.int32), _p(std_t, torch.float32, 'std_table'),
                                     _p(inv_t, torch.float32, 'inv_table'), _p(inv_m, torch.float32),
                                     _p(std_m, torch.float32), _p(ws), ws.numel(), B, N, _stream())
    _lib.check(rc, 'nhmc_mass_from_variance')
    return ws


def schedule_begin_mass(state, sigma_table, burn, epochs, sampling):
    lib = _lib.load()
    B = state['epoch'].numel()
    rc = lib.nhmc_schedule_begin_mass(_p(state['epoch'], torch.int32), _p(state['tau'], torch.float64),
                                      _p(state['eps'], torch.float64), _p(state['sigma_y'], torch.float64),
                                      _p(state['eps_eff'], torch.float64), _p(state['active'], torch.int32),
                                      _p(state['welford_on'], torch.int32), _p(sigma_table, torch.float64), burn, epochs,
                                      sampling, B, _stream())
    _lib.check(rc, 'nhmc_schedule_begin_mass')


def vq_nearest(z, codebook):
    """z [B, D, h, w], codebook [n_embed, D] -> (z_q = z + (e[k*] - z), k* int32 [B, h, w])."""
    lib = _lib.load()
    B, Dd = z.shape[0], z.shape[1]
    hw = z[0, 0].numel()
    if codebook.dim() != 2 or codebook.shape[1] != Dd:
        raise _lib.NhmcError(f'codebook {tuple(codebook.shape)} does not match latent channels {Dd}')
    zq = torch.empty_like(z)
    idx = torch.empty((B,) + tuple(z.shape[2:]), dtype=torch.int32, device=z.device)
    _lib.check(lib.nhmc_vq_nearest(_p(z, torch.float32, 'z'), _p(codebook, torch.float32, 'codebook'), _p(zq), _p(idx),
                                   B, Dd, hw, codebook.shape[0], _stream()), 'nhmc_vq_nearest')
    return zq, idx


def _gn_shape(shape, gamma, groups, film, pre):
    """-> (B, C, hw, the four conditioning arguments in ABI order: film, its row stride, pre, its row stride)"""
    B, Cc, hw = shape[0], shape[1], 1
    for d in shape[2:]:
        hw *= d
    if gamma.numel() != Cc or Cc % groups or hw % 4:
        raise _lib.NhmcError(f'fused GroupNorm: shape {tuple(shape)} / {groups} groups not covered (hw % 4 == 0, C % G == 0)')
    stride = pstride = 0
    if film is not None:
        if film.dim() != 2 or film.shape != (B, 2 * Cc) or film.stride(1) != 1:
            raise _lib.NhmcError('fused GroupNorm: film must be [B, 2C] (scale | shift) with unit inner stride')
        stride = film.stride(0)
    if pre is not None:
        if pre.stride(-1) != 1 or pre.shape not in ((Cc,), (B, Cc)):
            raise _lib.NhmcError('fused GroupNorm: pre must be float32 [C] or [B, C] with unit inner stride')
        pstride = pre.stride(0) if pre.dim() == 2 else 0
    return B, Cc, hw, (_p(film, torch.float32, 'film', contiguous=False), stride,
                       _p(pre, torch.float32, 'pre', contiguous=False), pstride)


def _ptr(t):
    """The unchecked address of a tensor: no wrapper uses it; tests/test_gn_onepass_gpu.py calls the raw ABI with it."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


GN_ONEPASS_NOWAIT = 1      # NHMC_GN_ONEPASS_NOWAIT of include/nhmc.h: tests only


def gn_onepass_splits(n, channels, groups, hw):
    """Split count of the one-pass GroupNorm kernels (csrc/gn_onepass.hip) for this shape; 0 when they do not cover it
    or NHMC_GN_ONEPASS=0 (the A/B switch, read per call) keeps the two-pass kernels."""
    if os.environ.get('NHMC_GN_ONEPASS', '1') == '0':
        return 0
    return _lib.load().nhmc_gn_onepass_splits(n, channels, groups, hw)


def gn_act_fwd(x, gamma, beta, groups, eps, act, film=None, pre=None, x2=None, flags=0, onepass=None):
    """GroupNorm of (x + pre) (+ FiLM) (+ SiLU) forward -> (y, ws, splits); ws feeds gn_act_bwd.
    x2 (optional, [B, C2, ...] with x's spatial shape): the input is cat([x, x2], dim=1) -- gamma, beta, film, pre are
    those of the concatenation -- and the result is (y, ws, splits, x_cat) with x_cat the concatenation itself, written
    by the same kernel; needs the one-pass kernels (gn_onepass_splits(...) > 0).
    onepass: None = the library's routing rule (nhmc_gn_onepass_prefers); True = one-pass wherever it covers the shape."""
    lib = _lib.load()
    if x2 is not None and (x2.shape[0] != x.shape[0] or x2.shape[2:] != x.shape[2:]):
        raise _lib.NhmcError('fused GroupNorm: the two sources must agree in batch and spatial shape')
    C1 = x.shape[1]
    shape = x.shape if x2 is None else (x.shape[0], C1 + x2.shape[1]) + tuple(x.shape[2:])
    B, Cc, hw, cond = _gn_shape(shape, gamma, groups, film, pre)
    one = gn_onepass_splits(B, Cc, groups, hw)
    if x2 is not None and not one:
        raise _lib.NhmcError('fused GroupNorm: two sources need the one-pass kernels, which do not cover this shape')
    if one and x2 is None and not onepass and not lib.nhmc_gn_onepass_prefers(0, B, Cc, groups, hw):
        one = 0
    y = torch.empty(shape, dtype=torch.float32, device=x.device)
    if one:
        ws = torch.empty(B * groups * (one + 1) * 2, dtype=torch.float64, device=x.device)   # partials, then the slab totals
        x_cat = torch.empty_like(y) if x2 is not None else None
        rc = lib.nhmc_gn_onepass_fwd(_p(x, torch.float32, 'x'), _p(x2, torch.float32, 'x2'), C1, _p(gamma, torch.float32, 'gamma'),
                                     _p(beta, torch.float32, 'beta'), *cond, float(eps), int(act),
                                     _p(y), _p(x_cat), _p(ws), int(flags), B, Cc, groups, hw, _stream())
        _lib.check(rc, 'nhmc_gn_onepass_fwd')
        return (y, ws, one) if x2 is None else (y, ws, one, x_cat)
    splits = lib.nhmc_gn_splits(B, Cc, groups, hw)
    ws = torch.empty(B * groups * splits * 2, dtype=torch.float64, device=x.device)
    rc = lib.nhmc_gn_act_fwd(_p(x, torch.float32, 'x'), _p(gamma, torch.float32, 'gamma'), _p(beta, torch.float32, 'beta'),
                             *cond, float(eps), int(act), _p(y), _p(ws), splits, B, Cc, groups,
                             hw, _stream())
    _lib.check(rc, 'nhmc_gn_act_fwd')
    return y, ws, splits


def gn_act_bwd(x, dy, gamma, beta, groups, eps, act, film, fwd_ws, splits, pre=None, add=None, c1=None, flags=0, onepass=None):
    """Input gradient of gn_act_fwd (parameters, FiLM and pre-bias terms are constants of the path).
    add (optional, x's shape): a second gradient of x, added in the same pass.
    c1 (optional, 0 < c1 < C): the gradient is returned as two contiguous tensors (dx[:, :c1], dx[:, c1:]); needs the
    one-pass kernels.  onepass: as in gn_act_fwd."""
    lib = _lib.load()
    B, Cc, hw, cond = _gn_shape(x.shape, gamma, groups, film, pre)
    one = gn_onepass_splits(B, Cc, groups, hw)
    if c1 is not None and not one:
        raise _lib.NhmcError('fused GroupNorm: a split gradient needs the one-pass kernels, which do not cover this shape')
    if one and c1 is None and not onepass and not lib.nhmc_gn_onepass_prefers(1, B, Cc, groups, hw):
        one = 0
    if add is not None and add.shape != x.shape:
        raise _lib.NhmcError('gn_act_bwd: `add` must have the shape of x')
    addp = _p(add, torch.float32, 'add')
    fwd_splits, own = splits, splits
    fwd_p = _p(fwd_ws, torch.float64)
    if fwd_ws.numel() == B * groups * (splits + 1) * 2:
        # a one-pass forward's workspace: its trailing one-split block (the slab totals) serves any backward, which
        # then chooses its own split count
        fwd_p, fwd_splits = C.c_void_p(fwd_ws.data_ptr() + B * groups * splits * 16), 1
        own = lib.nhmc_gn_splits(B, Cc, groups, hw)
    if one:
        ws = torch.empty(B * groups * one * 2, dtype=torch.float64, device=x.device)
        if c1 is None:
            dx1, dx2 = torch.empty_like(x), None
        else:
            dx1 = torch.empty((B, c1) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
            dx2 = torch.empty((B, Cc - c1) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        rc = lib.nhmc_gn_onepass_bwd(_p(x, torch.float32, 'x'), _p(dy, torch.float32, 'dy'), _p(gamma, torch.float32, 'gamma'),
                                     _p(beta, torch.float32, 'beta'), *cond, float(eps), int(act),
                                     fwd_p, int(fwd_splits), addp, _p(dx1), _p(dx2), Cc if c1 is None else int(c1),
                                     _p(ws), int(flags), B, Cc, groups, hw, _stream())
        _lib.check(rc, 'nhmc_gn_onepass_bwd')
        return dx1 if c1 is None else (dx1, dx2)
    ws = torch.empty(B * groups * own * 2, dtype=torch.float64, device=x.device)
    dx = torch.empty_like(x)
    rc = lib.nhmc_gn_act_bwd_fs(_p(x, torch.float32, 'x'), _p(dy, torch.float32, 'dy'), _p(gamma, torch.float32, 'gamma'),
                                _p(beta, torch.float32, 'beta'), *cond, float(eps), int(act),
                                fwd_p, int(fwd_splits), addp, _p(dx), _p(ws), own, B, Cc, groups, hw, _stream())
    _lib.check(rc, 'nhmc_gn_act_bwd_fs')
    return dx


def bias_add2(h, bias, other):
    """(h + bias[c]) + other for [B, C, ...] tensors: a convolution's bias folded into the residual add after it."""
    lib = _lib.load()
    if h.shape != other.shape or bias.numel() != h.shape[1]:
        raise _lib.NhmcError('bias_add2: shape mismatch')
    out = torch.empty_like(h)
    rc = lib.nhmc_bias_add2(_p(h, torch.float32, 'h'), _p(bias, torch.float32, 'bias'), _p(other, torch.float32, 'other'),
                            _p(out), h.shape[0], h.shape[1], h[0, 0].numel(), _stream())
    _lib.check(rc, 'nhmc_bias_add2')
    return out


_wino_u = {}          # (id(weight), backward) -> (weakref to it, its version counter, data_ptr, U on its device)
_wino_builds = 0


def wino_weight_builds():
    """How many times a transformed filter was built (tests: once per weight tensor and direction, again after an edit)."""
    return _wino_builds


def wino_weights(weight, backward=False):
    """U = G w G^T [16][c'][k'] of a [K, C, 3, 3] filter for conv3x3_wino (backward: the filter of the backward-data pass).
    Cached per LIVE weight tensor, version counter and storage address, like schedule.alpha_bar_table: the sampler's
    networks are frozen, so a run builds each U once (during the calls that precede a graph capture); an in-place edit or
    a move to another device rebuilds it."""
    global _wino_builds
    key = (id(weight), bool(backward))
    hit = _wino_u.get(key)
    if hit is not None and hit[0]() is weight and hit[1] == weight._version and hit[2] == weight.data_ptr():
        return hit[3]
    import weakref
    lib = _lib.load()
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise _lib.NhmcError(f'wino_weights: a [K, C, 3, 3] filter is needed, got {tuple(weight.shape)}')
    Kk, Cc = weight.shape[0], weight.shape[1]
    wd = weight.detach()
    u = torch.empty((16, Kk, Cc) if backward else (16, Cc, Kk), dtype=torch.float32, device=weight.device)
    _lib.check(lib.nhmc_wino_weights(_p(wd, torch.float32, 'weight'), _p(u), int(bool(backward)), Cc, Kk, _stream()),
               'nhmc_wino_weights')
    _wino_builds += 1
    for k in [k for k, v in _wino_u.items() if v[0]() is None]:
        del _wino_u[k]
    _wino_u[key] = (weakref.ref(weight), weight._version, weight.data_ptr(), u)
    return u


def _wino_narrow(w):
    """Images 32 and 16 wide run the kernel's narrow geometries, which have entries of their own (nhmc_conv3x3_wino_narrow*)."""
    return w in (32, 16)


def conv3x3_wino_covers(n, c, k, h, w):
    lib = _lib.load()
    return bool((lib.nhmc_conv3x3_wino_narrow_covers if _wino_narrow(w) else lib.nhmc_conv3x3_wino_covers)(n, c, k, h, w))


def conv3x3_wino_prefers(backward, n, c, k, h, w):
    """The library's routing rule (nhmc_conv3x3_wino_prefers); NHMC_WINO=0 (the A/B switch, read per call) answers no."""
    if os.environ.get('NHMC_WINO', '1') == '0':
        return False
    lib = _lib.load()
    prefers = lib.nhmc_conv3x3_wino_narrow_prefers if _wino_narrow(w) else lib.nhmc_conv3x3_wino_prefers
    return bool(prefers(int(bool(backward)), n, c, k, h, w))


def conv3x3_wino_k32_covers(n, c, k, h, w):
    """nhmc_conv3x3_wino_k32_covers: output-channel counts that are multiples of 32, every geometry; a superset of
    conv3x3_wino_covers, which keeps its answers."""
    return bool(_lib.load().nhmc_conv3x3_wino_k32_covers(n, c, k, h, w))


def conv3x3_wino_k32_prefers(backward, n, c, k, h, w):
    """The routing rule for k % 64 == 32 (nhmc_conv3x3_wino_k32_prefers); NHMC_WINO=0 answers no."""
    if os.environ.get('NHMC_WINO', '1') == '0':
        return False
    return bool(_lib.load().nhmc_conv3x3_wino_k32_prefers(int(bool(backward)), n, c, k, h, w))


def conv3x3_wino_skip_covers(n, c, k, h, w):
    """nhmc_conv3x3_wino_skip_covers: the wide geometry on eight waves (NHMC_WINO_WAVES is read per call) and NHMC_SKIP_BIAS,
    the A/B switch of the skip bias in the epilogue (read per call), not 0."""
    if os.environ.get('NHMC_SKIP_BIAS', '1') == '0' or _wino_narrow(w):
        return False
    return bool(_lib.load().nhmc_conv3x3_wino_skip_covers(n, c, k, h, w))


def conv3x3_wino(x, weight, bias=None, add=None, backward=False):
    """conv2d(x, weight, stride 1, padding 1) (+ bias[k]) (+ add) on the Winograd MFMA kernel; backward=True: the
    backward-data pass of that convolution, x being the output gradient [N, K, H, W] -> [N, C, H, W].
    An `add` of shape [N, K, H / 2, W / 2] stands for its nearest 2x upsample (conv3x3_wino_up, WINO_ADD_UP)."""
    lib = _lib.load()
    if x.dim() != 4 or weight.dim() != 4 or x.shape[1] != weight.shape[1 if not backward else 0]:
        raise _lib.NhmcError(f'conv3x3_wino: x {tuple(x.shape)} does not match the filter {tuple(weight.shape)}')
    u = wino_weights(weight, backward)
    N, Cc, H, W = x.shape
    Kk = u.shape[2]
    if add is not None and tuple(add.shape) == (N, Kk, H // 2, W // 2):
        return conv3x3_wino_up(x, weight, WINO_ADD_UP, bias, add, backward=backward)
    y = torch.empty((N, Kk, H, W), dtype=torch.float32, device=x.device)
    if (bias is not None and bias.numel() != Kk) or (add is not None and add.shape != y.shape):
        raise _lib.NhmcError('conv3x3_wino: bias / add do not match the output')
    entry = 'nhmc_conv3x3_wino_k32' if Kk % 64 else 'nhmc_conv3x3_wino_narrow' if _wino_narrow(W) else 'nhmc_conv3x3_wino'
    rc = getattr(lib, entry)(_p(x, torch.float32, 'x'), _p(u), _p(bias, torch.float32, 'bias'), _p(add, torch.float32, 'add'),
                             _p(y), N, Cc, Kk, H, W, 1, 1, _stream())
    _lib.check(rc, entry)
    return y


_thin_w = {}          # (id(weight), backward, thin output?) -> (weakref to it, its version counter, data_ptr, wp on its device)
_thin_builds = 0


def thin_weight_builds():
    """How many times a re-laid-out thin filter was built (tests: once per weight tensor and direction)."""
    return _thin_builds


def thin_in_weights(weight, backward=False, out=False):
    """wp [wide / 2][9 thin][2] of a filter for conv3x3_thin_in (nhmc_thin_in_weights): weight is [wide, thin, 3, 3] forward,
    [thin, wide, 3, 3] for backward=True (the backward-data pass of a convolution with a thin output).  Cached like
    wino_weights: per live weight tensor, version counter and storage address.
    out=True: gp [wide][9][2 ceil(thin / 2)] for conv3x3_thin_out (nhmc_thin_out_weights): weight is [thin, wide, 3, 3]
    forward, [wide, thin, 3, 3] for backward=True."""
    global _thin_builds
    key = (id(weight), bool(backward), bool(out))
    hit = _thin_w.get(key)
    if hit is not None and hit[0]() is weight and hit[1] == weight._version and hit[2] == weight.data_ptr():
        return hit[3]
    import weakref
    lib = _lib.load()
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise _lib.NhmcError(f'thin_in_weights: a [K, C, 3, 3] filter is needed, got {tuple(weight.shape)}')
    thin, wide = (weight.shape[0], weight.shape[1]) if bool(backward) != bool(out) else (weight.shape[1], weight.shape[0])
    if not 1 <= thin <= 8 or wide % 32:
        raise _lib.NhmcError(f'thin_in_weights: a thin side of at most 8 and a wide side that is a multiple of 32 are needed, '
                             f'got {thin} and {wide}')
    wd = weight.detach()
    wp = torch.empty((wide, 9, 2 * ((thin + 1) // 2)) if out else (wide // 2, 9 * thin, 2), dtype=torch.float32, device=weight.device)
    entry = 'nhmc_thin_out_weights' if out else 'nhmc_thin_in_weights'
    _lib.check(getattr(lib, entry)(_p(wd, torch.float32, 'weight'), _p(wp), int(bool(backward)), thin, wide, _stream()), entry)
    _thin_builds += 1
    for k in [k for k, v in _thin_w.items() if v[0]() is None]:
        del _thin_w[k]
    _thin_w[key] = (weakref.ref(weight), weight._version, weight.data_ptr(), wp)
    return wp


def conv3x3_thin_in_covers(n, c, k, h, w):
    return bool(_lib.load().nhmc_conv3x3_thin_in_covers(n, c, k, h, w))


def conv3x3_thin_in_prefers(backward, n, c, k, h, w):
    """The library's routing rule (nhmc_conv3x3_thin_in_prefers); NHMC_THIN_CONV=0 (the A/B switch, read per call) answers no."""
    if os.environ.get('NHMC_THIN_CONV', '1') == '0':
        return False
    return bool(_lib.load().nhmc_conv3x3_thin_in_prefers(int(bool(backward)), n, c, k, h, w))


def conv3x3_thin_in(x, weight, bias=None, backward=False):
    """conv2d(x, weight, stride 1, padding 1) (+ bias[k]) of a thin input x [N, C <= 8, H, W] to a wide output on the packed-FMA
    kernel (csrc/thin_conv.hip); backward=True: the backward-data pass of a convolution with a thin output, x being its
    output gradient [N, K <= 8, H, W] -> [N, C, H, W]."""
    lib = _lib.load()
    if x.dim() != 4 or weight.dim() != 4 or x.shape[1] != weight.shape[0 if backward else 1]:
        raise _lib.NhmcError(f'conv3x3_thin_in: x {tuple(x.shape)} does not match the filter {tuple(weight.shape)}')
    wp = thin_in_weights(weight, backward)
    N, Cc, H, W = x.shape
    Kk = 2 * wp.shape[0]
    if bias is not None and bias.numel() != Kk:
        raise _lib.NhmcError('conv3x3_thin_in: bias does not match the output')
    y = torch.empty((N, Kk, H, W), dtype=torch.float32, device=x.device)
    rc = lib.nhmc_conv3x3_thin_in(_p(x, torch.float32, 'x'), _p(wp), _p(bias, torch.float32, 'bias'), _p(y), N, Cc, Kk, H, W,
                                  1, 1, _stream())
    _lib.check(rc, 'nhmc_conv3x3_thin_in')
    return y


def conv3x3_thin_out_covers(n, c, k, h, w):
    return bool(_lib.load().nhmc_conv3x3_thin_out_covers(n, c, k, h, w))


def conv3x3_thin_out_prefers(backward, n, c, k, h, w):
    """nhmc_conv3x3_thin_out_prefers; NHMC_THIN_CONV=0 answers no."""
    if os.environ.get('NHMC_THIN_CONV', '1') == '0':
        return False
    return bool(_lib.load().nhmc_conv3x3_thin_out_prefers(int(bool(backward)), n, c, k, h, w))


def conv3x3_thin_out(x, weight, bias=None, backward=False):
    """conv2d(x, weight, stride 1, padding 1) (+ bias[k]) of a wide input x [N, C, H, W] to a thin output (K <= 8) on the
    packed-FMA kernel; backward=True: the backward-data pass of a convolution with a thin input, x being its output gradient
    [N, K, H, W] (K wide) -> [N, C <= 8, H, W]."""
    lib = _lib.load()
    if x.dim() != 4 or weight.dim() != 4 or x.shape[1] != weight.shape[0 if backward else 1]:
        raise _lib.NhmcError(f'conv3x3_thin_out: x {tuple(x.shape)} does not match the filter {tuple(weight.shape)}')
    gp = thin_in_weights(weight, backward, out=True)
    N, Cc, H, W = x.shape
    Kk = weight.shape[1 if backward else 0]
    if bias is not None and bias.numel() != Kk:
        raise _lib.NhmcError('conv3x3_thin_out: bias does not match the output')
    y = torch.empty((N, Kk, H, W), dtype=torch.float32, device=x.device)
    rc = lib.nhmc_conv3x3_thin_out(_p(x, torch.float32, 'x'), _p(gp), _p(bias, torch.float32, 'bias'), _p(y), N, Cc, Kk, H, W,
                                   1, 1, _stream())
    _lib.check(rc, 'nhmc_conv3x3_thin_out')
    return y


def conv3x3_wino_skip(x, weight, bias, add, add_bias):
    """conv3x3_wino(x, weight, bias, add + add_bias[k]) without the pass that adds add_bias to `add` [N, K, H, W]: the
    kernel's epilogue forms (acc + bias[k]) + (add + add_bias[k]), the same bits (nhmc_conv3x3_wino_skip; forward filter,
    where conv3x3_wino_skip_covers)."""
    lib = _lib.load()
    if x.dim() != 4 or weight.dim() != 4 or x.shape[1] != weight.shape[1]:
        raise _lib.NhmcError(f'conv3x3_wino_skip: x {tuple(x.shape)} does not match the filter {tuple(weight.shape)}')
    u = wino_weights(weight, False)
    N, Cc, H, W = x.shape
    Kk = u.shape[2]
    y = torch.empty((N, Kk, H, W), dtype=torch.float32, device=x.device)
    if (bias is not None and bias.numel() != Kk) or add is None or add.shape != y.shape or add_bias is None or add_bias.numel() != Kk:
        raise _lib.NhmcError('conv3x3_wino_skip: bias / add / add_bias do not match the output')
    rc = lib.nhmc_conv3x3_wino_skip(_p(x, torch.float32, 'x'), _p(u), _p(bias, torch.float32, 'bias'), _p(add, torch.float32, 'add'),
                                    _p(add_bias, torch.float32, 'add_bias'), _p(y), N, Cc, Kk, H, W, _stream())
    _lib.check(rc, 'nhmc_conv3x3_wino_skip')
    return y


WINO_IN_UP, WINO_ADD_UP, WINO_OUT_POOL = 1, 2, 4      # NHMC_WINO_* of include/nhmc.h


def conv3x3_wino_up_covers(n, c, k, h, w):
    """nhmc_conv3x3_wino_up_covers at the convolution's own (upsampled) shape: the wide geometry on eight waves
    (NHMC_WINO_WAVES is read per call) and NHMC_WINO_UP, the A/B switch of the fused upsample forms, not 0."""
    if os.environ.get('NHMC_WINO_UP', '1') == '0' or _wino_narrow(w):
        return False
    return bool(_lib.load().nhmc_conv3x3_wino_up_covers(n, c, k, h, w))


def conv3x3_wino_up(x, weight, mode, bias=None, add=None, backward=False):
    """conv3x3_wino next to a nearest 2x upsample that never reaches memory (nhmc_conv3x3_wino_up).  WINO_IN_UP: x is the
    low-res tensor [N, C, H / 2, W / 2]; WINO_ADD_UP: add is [N, K, H / 2, W / 2]; WINO_OUT_POOL: the result is the 2 x 2
    block sum [N, K, H / 2, W / 2] of the convolution's output (the gradient of an upsampled input)."""
    lib = _lib.load()
    if x.dim() != 4 or weight.dim() != 4 or x.shape[1] != weight.shape[1 if not backward else 0]:
        raise _lib.NhmcError(f'conv3x3_wino_up: x {tuple(x.shape)} does not match the filter {tuple(weight.shape)}')
    u = wino_weights(weight, backward)
    N, Cc = x.shape[0], x.shape[1]
    H, W = (2 * x.shape[2], 2 * x.shape[3]) if mode == WINO_IN_UP else (x.shape[2], x.shape[3])
    Kk = u.shape[2]
    y = torch.empty((N, Kk, H // 2, W // 2) if mode == WINO_OUT_POOL else (N, Kk, H, W), dtype=torch.float32, device=x.device)
    if (bias is not None and bias.numel() != Kk) or (add is not None and tuple(add.shape) != (N, Kk, H // 2, W // 2)):
        raise _lib.NhmcError('conv3x3_wino_up: bias / add do not match the output')
    rc = lib.nhmc_conv3x3_wino_up(_p(x, torch.float32, 'x'), _p(u), _p(bias, torch.float32, 'bias'), _p(add, torch.float32, 'add'),
                                  _p(y), N, Cc, Kk, H, W, int(mode), _stream())
    _lib.check(rc, 'nhmc_conv3x3_wino_up')
    return y


def psnr(xt, x_orig):
    lib = _lib.load()
    B, N = _chains_elems(xt)
    ws = torch.empty(B * lib.nhmc_data_tiles(N), dtype=torch.float64, device=xt.device)
    out = torch.empty(B, dtype=torch.float32, device=xt.device)
    _lib.check(lib.nhmc_psnr(_p(xt, torch.float32, 'xt'), _p(x_orig, torch.float32, 'x_orig'), _p(out), _p(ws),
                             B, N, _stream()), 'nhmc_psnr')
    return out


# ---- report stage (nhmc.h "Report stage") ------------------------------------------------------
def _sample_block(samples, x_orig=None):
    """samples [B, S, C, H, W] (and x_orig [B, C, H, W]) -> (B, S, C, H, W)"""
    if samples.dim() != 5:
        raise _lib.NhmcError(f'samples must be [chains, samples, C, H, W], got {tuple(samples.shape)}')
    if x_orig is not None and (x_orig.dim() != 4 or x_orig.shape[0] != samples.shape[0] or x_orig.shape[1:] != samples.shape[2:]):
        raise _lib.NhmcError(f'x_orig {tuple(x_orig.shape)} does not match samples {tuple(samples.shape)}')
    return tuple(samples.shape)


def psnr_samples(samples, x_orig):
    """PSNR of samples[b, j] against x_orig[b] -> float32 [B, S], the bits `psnr` gives pair by pair, in one launch pair."""
    lib = _lib.load()
    B, S, Cc, H, W = _sample_block(samples, x_orig)
    N = Cc * H * W
    ws = torch.empty(B * S * lib.nhmc_data_tiles(N), dtype=torch.float64, device=samples.device)
    out = torch.empty((B, S), dtype=torch.float32, device=samples.device)
    _lib.check(lib.nhmc_psnr_samples(_p(samples, torch.float32, 'samples'), _p(x_orig, torch.float32, 'x_orig'), _p(out),
                                     _p(ws), B, S, N, _stream()), 'nhmc_psnr_samples')
    return out


def ssim_ws(n_total_samples, Cc, H, W, device):
    return torch.empty(_lib.load().nhmc_ssim_ws_bytes(n_total_samples, Cc, H, W) // 8, dtype=torch.float64, device=device)


def sample_range(samples, ws=None):
    """max - min of every transformed sample over all its channels -> float32 [B, S] (the reference's `data_range`)."""
    lib = _lib.load()
    B, S, Cc, H, W = _sample_block(samples)
    ws = ssim_ws(B * S, Cc, H, W, samples.device) if ws is None else ws
    out = torch.empty((B, S), dtype=torch.float32, device=samples.device)
    _lib.check(lib.nhmc_sample_range(_p(samples, torch.float32, 'samples'), _p(out), _p(ws, torch.float64, 'ws'), B * S,
                                     Cc * H * W, _stream()), 'nhmc_sample_range')
    return out


def ssim(samples, x_orig, data_range=None):
    """skimage's default SSIM (channel_axis=0) of samples[b, j] against x_orig[b] with data_range = the sample's own range
    -> float64 [B, S]."""
    lib = _lib.load()
    B, S, Cc, H, W = _sample_block(samples, x_orig)
    ws = ssim_ws(B * S, Cc, H, W, samples.device)
    if data_range is None:
        data_range = sample_range(samples, ws)
    elif data_range.shape != (B, S):
        raise _lib.NhmcError(f'data_range must be [{B}, {S}]')
    out = torch.empty((B, S), dtype=torch.float64, device=samples.device)
    _lib.check(lib.nhmc_ssim(_p(samples, torch.float32, 'samples'), _p(x_orig, torch.float32, 'x_orig'),
                             _p(data_range, torch.float32, 'data_range'), _p(out), _p(ws, torch.float64, 'ws'), B, S, Cc, H, W,
                             _stream()), 'nhmc_ssim')
    return out


def sample_moments(samples):
    """-> (mean [B, C, H, W] of the raw samples, std_map [B, H, W] of the transformed ones, minmax [B, 2] of the map)"""
    lib = _lib.load()
    B, S, Cc, H, W = _sample_block(samples)
    dev = samples.device
    mean = torch.empty((B, Cc, H, W), dtype=torch.float32, device=dev)
    std_map = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    minmax = torch.empty((B, 2), dtype=torch.float32, device=dev)
    ws = torch.empty(B * lib.nhmc_moments_tiles(H * W) * 2, dtype=torch.float64, device=dev)
    _lib.check(lib.nhmc_sample_moments(_p(samples, torch.float32, 'samples'), _p(mean), _p(std_map), _p(minmax), _p(ws),
                                       B, S, Cc, H, W, _stream()), 'nhmc_sample_moments')
    return mean, std_map, minmax


def std_map_normalise(std_map, minmax):
    """(std_map - min) / (max - min) per chain -> float32 [B, H, W]"""
    lib = _lib.load()
    if std_map.dim() != 3 or minmax.shape != (std_map.shape[0], 2):
        raise _lib.NhmcError('std_map must be [B, H, W] and minmax [B, 2]')
    out = torch.empty_like(std_map)
    _lib.check(lib.nhmc_std_map_normalise(_p(std_map, torch.float32, 'std_map'), _p(minmax, torch.float32, 'minmax'), _p(out),
                                          std_map.shape[0], std_map.shape[1] * std_map.shape[2], _stream()),
               'nhmc_std_map_normalise')
    return out


def _pooled(samples, n_replicas, what, x_orig=None):
    """-> (G, K, S, N): the images, replicas, samples per chain and elements of a [G * K, S, C, H, W] block on the GPU,
    after checking it and an x_orig [G, C, H, W] given with it."""
    if not samples.is_cuda:
        raise _lib.NhmcError(f'{what}: samples must live on the GPU (got {samples.device}); libnhmc has no CPU path')
    B, S, Cc, H, W = _sample_block(samples)
    K = int(n_replicas)
    if K < 1 or B % K:
        raise _lib.NhmcError(f'{what}: {B} chains are not a multiple of {n_replicas} replicas')
    G = B // K
    if x_orig is not None and (x_orig.dim() != 4 or x_orig.shape[0] != G or x_orig.shape[1:] != samples.shape[2:]):
        raise _lib.NhmcError(f'x_orig {tuple(x_orig.shape)} does not match {G} images of samples {tuple(samples.shape)}')
    return G, K, S, Cc * H * W


def chain_diag(samples, n_replicas, rhat_threshold=1.1):
    """Split R-hat and ESS per element over the replicas of every image (nhmc.h "Convergence of replica chains").
    samples [G * n_replicas, S, C, H, W], chain g * n_replicas + r being replica r of image g
    -> (rhat [G, C, H, W], ess [G, C, H, W] float32, summary [G, 6] float64)."""
    G, K, S, N = _pooled(samples, n_replicas, 'chain_diag')
    lib = _lib.load()
    dev, img = samples.device, (G,) + tuple(samples.shape[2:])
    rhat = torch.empty(img, dtype=torch.float32, device=dev)
    ess = torch.empty(img, dtype=torch.float32, device=dev)
    summary = torch.empty((G, 6), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.nhmc_chain_diag_ws_bytes(G, N) // 8, dtype=torch.float64, device=dev)
    _lib.check(lib.nhmc_chain_diag(_p(samples, torch.float32, 'samples'), _p(rhat), _p(ess), _p(summary), _p(ws), G, K, S, N,
                                   float(rhat_threshold), _stream()), 'nhmc_chain_diag')
    return rhat, ess, summary


def calibration(samples, x_orig, n_replicas=1):
    """Rank and z-score of the original among an image's pooled draws (nhmc.h "Calibration of the posterior samples").
    samples [G * n_replicas, S, C, H, W], chain g * n_replicas + r being replica r of image g, and x_orig [G, C, H, W]
    -> (z [G, C, H, W] float32, counts [G, C, H, W] int32 = below + 65536 * equal, hist [G, n + 1] int64 with
    n = n_replicas * S, summary [G, 8] float64)."""
    if x_orig is None:
        raise _lib.NhmcError('calibration: x_orig is needed')
    G, K, S, N = _pooled(samples, n_replicas, 'calibration', x_orig)
    lib = _lib.load()
    dev, img = samples.device, (G,) + tuple(samples.shape[2:])
    z = torch.empty(img, dtype=torch.float32, device=dev)
    counts = torch.empty(img, dtype=torch.int32, device=dev)
    hist = torch.empty((G, K * S + 1), dtype=torch.int64, device=dev)
    summary = torch.empty((G, 8), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.nhmc_calibration_ws_bytes(G, N) // 8, dtype=torch.float64, device=dev)
    _lib.check(lib.nhmc_calibration(_p(samples, torch.float32, 'samples'), _p(x_orig, torch.float32, 'x_orig'), _p(z),
                                    _p(counts), _p(hist), _p(summary), _p(ws), G, K, S, N, _stream()), 'nhmc_calibration')
    return z, counts, hist, summary


def credible(samples, x_orig, n_replicas=1, k=1):
    """Order statistics of an image's pooled draws (nhmc.h "Credible interval and median of the posterior samples").
    samples [G * n_replicas, S, C, H, W], chain g * n_replicas + r being replica r of image g, x_orig [G, C, H, W] or None,
    1 <= k <= n // 2 with n = n_replicas * S -> (lower, median, upper [G, C, H, W] float32: d_(k), the median and
    d_(n+1-k) of the n draws in torch.sort's order, summary [G, 6] float64)."""
    G, K, S, N = _pooled(samples, n_replicas, 'credible', x_orig)
    lib = _lib.load()
    dev = samples.device
    lower, median, upper = (torch.empty((G,) + tuple(samples.shape[2:]), dtype=torch.float32, device=dev) for _ in range(3))
    summary = torch.empty((G, 6), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.nhmc_credible_ws_bytes(G, N) // 8, dtype=torch.float64, device=dev)
    _lib.check(lib.nhmc_credible(_p(samples, torch.float32, 'samples'), _p(x_orig, torch.float32, 'x_orig'), _p(lower),
                                 _p(median), _p(upper), _p(summary), _p(ws), G, K, S, N, int(k), _stream()), 'nhmc_credible')
    return lower, median, upper, summary


def sample_gram(samples, x_orig, n_replicas=1):
    """Gram matrix of an image's pooled draws about the first one (nhmc.h "Principal components of the posterior samples").
    samples [G * n_replicas, S, C, H, W], chain g * n_replicas + r being replica r of image g, x_orig [G, C, H, W] or None,
    2 <= n = n_replicas * S <= 256 -> [G, n, n] float64: rows u_1 ... u_{n-1} = d_2 - d_1 ... d_n - d_1 and u_n = t - d_1
    (NaN without x_orig), exactly symmetric."""
    G, K, S, N = _pooled(samples, n_replicas, 'sample_gram', x_orig)
    lib = _lib.load()
    n, dev = K * S, samples.device
    gram = torch.empty((G, n, n), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.nhmc_sample_gram_ws_bytes(G, n, N) // 8, dtype=torch.float64, device=dev)
    _lib.check(lib.nhmc_sample_gram(_p(samples, torch.float32, 'samples'), _p(x_orig, torch.float32, 'x_orig'), _p(gram),
                                    _p(ws), G, K, S, N, _stream()), 'nhmc_sample_gram')
    return gram


def sample_project(samples, coef, n_replicas=1):
    """Images from coefficients over an image's pooled draws: out[g, j] = sum_i coef[g, j, i] (d_i - d_1) in fp64, rounded
    once.  samples as for `sample_gram`, coef [G, J, n] float64 with 1 <= J <= 8 -> [G, J, C, H, W] float32."""
    G, K, S, N = _pooled(samples, n_replicas, 'sample_project')
    lib = _lib.load()
    n = K * S
    if coef.dim() != 3 or coef.shape[0] != G or coef.shape[2] != n:
        raise _lib.NhmcError(f'coef {tuple(coef.shape)} does not match {G} images of {n} pooled draws')
    J = coef.shape[1]
    out = torch.empty((G, J) + tuple(samples.shape[2:]), dtype=torch.float32, device=samples.device)
    _lib.check(lib.nhmc_sample_project(_p(samples, torch.float32, 'samples'), _p(coef, torch.float64, 'coef'), _p(out),
                                       G, K, S, J, N, _stream()), 'nhmc_sample_project')
    return out


# ---- a1-------------------------------------------------------------------------------------
def randn_philox(shape, seed, chain_id0, draw, scale=1.0, device='cuda', out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    B, N = _chains_elems(out)
    _lib.check(lib.nhmc_randn_philox(_p(out, torch.float32), int(seed), int(chain_id0), int(draw), float(scale),
                                     B, N, _stream()), 'nhmc_randn_philox')
    return out


def uniform_philox(n_chains, seed, chain_id0, draw, device='cuda'):
    lib = _lib.load()
    out = torch.empty(n_chains, dtype=torch.float32, device=device)
    _lib.check(lib.nhmc_uniform_philox(_p(out), int(seed), int(chain_id0), int(draw), n_chains, _stream()),
               'nhmc_uniform_philox')
    return out


def copy_probe(src, dst):
    """Streaming copy with the fused update's access pattern (measurement aid for bench.py's copy ceiling)."""
    lib = _lib.load()
    if src.numel() != dst.numel():
        raise _lib.NhmcError('copy_probe: size mismatch')
    _lib.check(lib.nhmc_copy_probe(_p(src, torch.float32, 'src'), _p(dst, torch.float32, 'dst'), src.numel(), _stream()),
               'nhmc_copy_probe')
    return dst
