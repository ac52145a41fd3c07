import sys, time, torch
sys.path.insert(0, '.')
import nhmc.kernels as K
from nhmc import operators
dev = torch.device('cuda')
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
def timeit(f, n=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
x = K.randn_philox((B, 3, 256, 256), 1, 0, 0)
T = B * 3 * 256 * 256 * 4
# Fourier sampling (operators.FourierSampling): mri4 = the centred 2-D DFT kept on 64 of 256 k-space columns.  Data term +
# last VJP, 10 warm-up calls then 100 timed ones between two events, three windows alternating in this process with the same
# term written with torch.fft + autograd (its last-step VJP by autograd through the clipped DDIM mix); medians.  FLOP model
# per plane at n = d: 2 d d 2d + 8 (2 d d d) + 2 d d 2d = 24 d^3 (stage 1, the two four-product stages, stage 4).
# `python tools/ops_bench.py 64 fourier` runs this leg alone.
def timed(f, warm=10, n=100):
    for _ in range(warm): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
def fourier_leg():
    d = 256
    om = operators.build_operator('mri4', 3, d, dev, generator=torch.Generator().manual_seed(5678))
    e6 = K.randn_philox((B, 6, d, d), 1, 0, 2)
    ge = torch.zeros_like(e6)
    at = torch.full((B,), 0.5214230418, device=dev)
    an = torch.ones(B, device=dev)
    cur = K.ddim_mix_fwd(x, e6, at, an, final_clip=True)['xt_next']
    ym = K.randn_philox((B, om.M), 1, 0, 5)
    W, meas = om.W, om.W > 0
    yc = torch.complex(*ym.reshape(B, 3, 2, d, d).unbind(2))
    a_, b_ = at.view(B, 1, 1, 1), an.view(B, 1, 1, 1)
    def torch_term():
        xl, el = x.detach().requires_grad_(True), e6.detach().requires_grad_(True)
        x0 = ((xl - el[:, :3] * (1 - a_).sqrt()) / a_.sqrt()).clamp(-1, 1)   # the last DDIM step (eta = 0), then the final clip
        dec = (b_.sqrt() * x0 + (1 - b_).sqrt() * el[:, :3]).clamp(-1, 1)
        Y = torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(dec, dim=(-2, -1)), norm='ortho'), dim=(-2, -1))
        r = torch.where(meas, yc - W * Y, torch.zeros((), dtype=yc.dtype, device=dev))
        loss = (r.real ** 2 + r.imag ** 2).sum()
        return torch.autograd.grad(loss, (xl, el))
    ours, theirs = [], []
    for _ in range(3):
        ours.append(timed(lambda: om.fused_last_vjp(x, e6, at, an, ym, g_e_out=ge, xt_next=cur)))
        theirs.append(timed(torch_term))
    ms, mst = sorted(ours)[1], sorted(theirs)[1]
    msD, msH = timed(lambda: om.data_term(x, ym, True)), timed(lambda: om.H(x))
    fl = B * 3 * 24 * d ** 3
    print(f'mri4 (64 of 256 columns) B={B}: data term + last VJP {ms*1e3:.1f} us {fl/ms/1e9:.1f} TFLOP/s ({fl/1e9:.1f} GFLOP; windows '
          f'{", ".join(f"{v*1e3:.1f}" for v in ours)}), torch.fft + autograd {mst*1e3:.1f} us ({mst/ms:.2f} x ours; windows '
          f'{", ".join(f"{v*1e3:.1f}" for v in theirs)});  data term {msD*1e3:.1f} us, H {msH*1e3:.1f} us')
# Modulated Fourier operators (operators.ModulatedFourier): mcmri4 with 8 coils (linear) and cdp4 (modulus), timed as the
# Fourier leg is: data term + last VJP, 10 warm-up calls then 100 timed ones between two events, three windows alternating
# with the same term written with torch.fft + autograd; medians; then the data term alone and H.  FLOP model: the chain runs
# on the real and the imaginary plane of every modulated image, 2 x 24 d^3 = 48 d^3 per (plane, map); a complex-input chain
# would need 32 d^3 (a complex product is four real ones of 2 d^3 FLOP, two per transform, forward and adjoint).
# `python tools/ops_bench.py 64 modfourier` runs this leg alone.
def modfourier_leg():
    d = 256
    e6 = K.randn_philox((B, 6, d, d), 1, 0, 2)
    ge = torch.zeros_like(e6)
    at = torch.full((B,), 0.5214230418, device=dev)
    an = torch.ones(B, device=dev)
    cur = K.ddim_mix_fwd(x, e6, at, an, final_clip=True)['xt_next']
    a_, b_ = at.view(B, 1, 1, 1), an.view(B, 1, 1, 1)
    for deg, label in (('mcmri4', 'mcmri4, 8 coils (64 of 256 columns)'), ('cdp4', 'cdp4 (4 masks, modulus)')):
        om = operators.build_operator(deg, 3, d, dev, generator=torch.Generator().manual_seed(5678), n_coils=8)
        Km = om.maps.shape[0]
        ym = K.randn_philox((B, om.M), 1, 0, 5)
        if om.modulus: ym = ym.abs()
        W, meas, S = om.W, om.W > 0, om.maps.to(dev)
        yo = om._observation(ym, x.shape)
        yc = yo if om.modulus else torch.complex(*yo.unbind(3))
        def torch_term():
            xl, el = x.detach().requires_grad_(True), e6.detach().requires_grad_(True)
            x0 = ((xl - el[:, :3] * (1 - a_).sqrt()) / a_.sqrt()).clamp(-1, 1)   # the last DDIM step (eta = 0), then the final clip
            dec = (b_.sqrt() * x0 + (1 - b_).sqrt() * el[:, :3]).clamp(-1, 1)
            z = S * dec[:, :, None]
            Y = torch.fft.fftshift(torch.fft.fft2(torch.fft.ifftshift(z, dim=(-2, -1)), norm='ortho'), dim=(-2, -1))
            if om.modulus:
                loss = (torch.where(meas, yc - W * Y.abs(), torch.zeros((), device=dev)) ** 2).sum()
            else:
                r = torch.where(meas, yc - W * Y, torch.zeros((), dtype=yc.dtype, device=dev))
                loss = (r.real ** 2 + r.imag ** 2).sum()
            return torch.autograd.grad(loss, (xl, el))
        ours, theirs = [], []
        for _ in range(3):
            ours.append(timed(lambda: om.fused_last_vjp(x, e6, at, an, ym, g_e_out=ge, xt_next=cur)))
            theirs.append(timed(torch_term))
        ms, mst = sorted(ours)[1], sorted(theirs)[1]
        msD, msH = timed(lambda: om.data_term(x, ym, True)), timed(lambda: om.H(x))
        fl = B * 3 * Km * 48 * d ** 3
        print(f'{label} B={B}: data term + last VJP {ms*1e3:.1f} us {fl/ms/1e9:.1f} TFLOP/s ({fl/1e9:.1f} GFLOP at 48 d^3 per plane and map; '
              f'windows {", ".join(f"{v*1e3:.1f}" for v in ours)}), torch.fft + autograd {mst*1e3:.1f} us ({mst/ms:.2f} x ours; windows '
              f'{", ".join(f"{v*1e3:.1f}" for v in theirs)});  data term {msD*1e3:.1f} us, H {msH*1e3:.1f} us', flush=True)
        del om, ym, yo, yc
        torch.cuda.empty_cache()
if len(sys.argv) > 2 and sys.argv[2] == 'fourier':
    fourier_leg()
    sys.exit(0)
if len(sys.argv) > 2 and sys.argv[2] == 'modfourier':
    modfourier_leg()
    sys.exit(0)
op = operators.build_operator('deblur_aniso', 3, 256, dev)
y = K.randn_philox((B, 3, 256, 256), 1, 0, 1).reshape(B, -1)
ms = timeit(lambda: op.data_term(x, y, True), 10)
nprod = 4 if op.projected else 8
fl = nprod * B * 3 * 2 * 256 ** 3
print(f'aniso data term B={B}: {ms:.3f} ms  {fl/ms/1e9:.1f} TFLOP/s  ({fl/1e9:.1f} GFLOP executed, {nprod} products)')
ms = timeit(lambda: op.H(x), 10)
print(f'aniso H B={B}: {ms:.3f} ms  {4 * B * 3 * 2 * 256 ** 3/ms/1e9:.1f} TFLOP/s')
op4 = operators.build_operator('sr4', 3, 256, dev)
y4 = torch.randn(B, op4.M, device=dev)
ms = timeit(lambda: op4.data_term(x, y4, True))
print(f'sr4 data term B={B}: {ms*1e3:.1f} us  {(2*T)/ms/1e6:.0f} GB/s (2T)')
op16 = operators.build_operator('sr16', 3, 256, dev)
y16 = torch.randn(B, op16.M, device=dev)
ms = timeit(lambda: op16.data_term(x, y16, True))
print(f'sr16 data term B={B}: {ms*1e3:.1f} us  {(2*T)/ms/1e6:.0f} GB/s (2T)')
opi = operators.build_operator('inpaint_random', 3, 256, dev)
yi = torch.randn(B, opi.M, device=dev)
ms = timeit(lambda: opi.data_term(x, yi, True))
print(f'inpaint data term B={B}: {ms*1e3:.1f} us  {(2*T)/ms/1e6:.0f} GB/s (2T dense)')
for deg, nbytes in (('cs4', None), ('sr_bicubic4', None), ('color', None), ('deblur_gauss', None)):
    o = operators.build_operator(deg, 3, 256, dev)
    yy = torch.randn(B, o.M, device=dev)
    ms = timeit(lambda: o.data_term(x, yy, True), 10)
    print(f'{deg} data term B={B}: {ms*1e3:.1f} us  ({T/ms/1e6:.0f} GB/s per T moved)')
# fused (data term + last DDIM-step VJP) kernels: R xt, R e[:C], W g_xt, W g_e[:C] = 4T
e6 = K.randn_philox((B, 6, 256, 256), 1, 0, 2)
ge = torch.zeros_like(e6)
at = torch.full((B,), 0.5214230418, device=dev)
an = torch.ones(B, device=dev)
for name, o, yy in (('inpaint', opi, yi), ('sr4', op4, y4), ('sr16', op16, y16)):
    ms = timeit(lambda: o.fused_last_vjp(x, e6, at, an, yy, g_e_out=ge))
    print(f'{name} fused last VJP B={B}: {ms*1e3:.1f} us  {(4*T)/ms/1e6:.0f} GB/s (4T)')
cur = K.ddim_mix_fwd(x, e6, at, an, final_clip=True)['xt_next']
def two_kernel():
    l, g = op.data_term(cur, y, apply_clip=False)
    return K.ddim_mix_bwd(g, x, e6, at, an, final_clip=True, g_e_out=ge)
ms2 = timeit(two_kernel, 10)
ms1 = timeit(lambda: op.fused_last_vjp(x, e6, at, an, y, g_e_out=ge, xt_next=cur), 10)
print(f'aniso data term + last VJP B={B}: two kernels {ms2*1e3:.1f} us, fused epilogue {ms1*1e3:.1f} us')
opp = operators.build_operator('deblur_aniso', 3, 256, dev, spectral_projected=True)
ms = timeit(lambda: opp.data_term(x, y, True), 10)
msv = timeit(lambda: opp.fused_last_vjp(x, e6, at, an, y, g_e_out=ge, xt_next=cur), 10)
flp = 4 * B * 3 * 2 * 256 ** 3
print(f'aniso projected (4 products) B={B}: data term {ms*1e3:.1f} us {flp/ms/1e9:.1f} TFLOP/s, + last VJP {msv*1e3:.1f} us {flp/msv/1e9:.1f} TFLOP/s')
# the two nonlinear operators.  HDR fused kernel: R xt, R e[:C], R y, W g_xt, W g_e[:C] = 5T, the inpainting fused kernel's
# traffic with a dense observation -- compare against the inpaint line of THIS run.  Phase retrieval (n = 384): FLOP model
# per plane 2 d d 2n + 8 (2 n n d) + 2 d d 2n (stage 1, the two four-product stages, stage 4).
oph = operators.build_operator('hdr', 3, 256, dev)
yh = torch.randn(B, oph.M, device=dev)
ms = timeit(lambda: oph.fused_last_vjp(x, e6, at, an, yh, g_e_out=ge))
msi = timeit(lambda: opi.fused_last_vjp(x, e6, at, an, yi, g_e_out=ge))
print(f'hdr fused last VJP B={B}: {ms*1e3:.1f} us  {(5*T)/ms/1e6:.0f} GB/s (5T);  inpaint fused, same session: {msi*1e3:.1f} us')
ms = timeit(lambda: oph.data_term(x, yh, True))
print(f'hdr data term B={B}: {ms*1e3:.1f} us  {(3*T)/ms/1e6:.0f} GB/s (3T)')
opf = operators.build_operator('phase_retrieval', 3, 256, dev)
d_, n_ = 256, opf.n
yf = torch.rand(B, opf.M, device=dev)
flf = B * 3 * (2 * (2 * d_ * d_ * 2 * n_) + 8 * (2 * n_ * n_ * d_))
ms = timeit(lambda: opf.data_term(x, yf, True), 10)
msv = timeit(lambda: opf.fused_last_vjp(x, e6, at, an, yf, g_e_out=ge, xt_next=cur), 10)
msa = timeit(lambda: op.fused_last_vjp(x, e6, at, an, y, g_e_out=ge, xt_next=cur), 10)
print(f'phase_retrieval B={B}: data term {ms*1e3:.1f} us {flf/ms/1e9:.1f} TFLOP/s, + last VJP {msv*1e3:.1f} us {flf/msv/1e9:.1f} TFLOP/s '
      f'({flf/1e9:.1f} GFLOP);  deblur_aniso + last VJP, same session: {msa*1e3:.1f} us')
ms = timeit(lambda: opf.H(x), 10)
print(f'phase_retrieval H B={B}: {ms*1e3:.1f} us')
# the general 2-D PSF blur (deblur_motion): the seeded sparse camera-shake PSF and a dense K = 61 one.  Yardstick in the
# same process with windows alternating: torch's depthwise F.conv2d for H, its autograd for the data term.  Bound: the tap
# loop moves one LDS dword per FMA and ds_read_b32 runs at 32 lanes/clk/CU -> 256 CUs x 32 x 2.4 GHz = 19.7 T FMA/s.
import torch.nn.functional as F
def alternate(f, g, windows=3, n=5):
    a, b = [], []
    for _ in range(windows):
        a.append(timeit(f, n)); b.append(timeit(g, n))
    return sorted(a)[len(a) // 2], sorted(b)[len(b) // 2]
gen = torch.Generator().manual_seed(5678)
dense = torch.rand(61, 61, generator=gen) + 0.1
for name, psf in (('deblur_motion sparse', operators.motion_kernel(61, 0.5, gen)), ('dense K=61', dense / dense.sum())):
    om = operators.Blur2D(psf, 3, 256, dev)
    Tn = om.taps()[1].numel()
    wt = psf.to(dev)[None, None].expand(3, 1, 61, 61).contiguous()
    ym = K.randn_philox((B, 3, 256, 256), 1, 0, 3)
    def torch_H():
        return F.conv2d(x, wt, padding=30, groups=3)
    def torch_data():
        xl = x.detach().requires_grad_(True)
        loss = ((ym - F.conv2d(xl.clamp(-1, 1), wt, padding=30, groups=3)) ** 2).sum()
        return torch.autograd.grad(loss, xl)
    fma = B * 3 * 256 * 256 * Tn
    msH, msHt = alternate(lambda: om.H(x), torch_H)
    msD, msDt = alternate(lambda: om.data_term(x, ym, True), torch_data)
    msV = timeit(lambda: om.fused_last_vjp(x, e6, at, an, ym, g_e_out=ge, xt_next=cur), 5)
    print(f'{name} (T = {Tn}) B={B}: H {msH*1e3:.1f} us ({fma/msH/1e9:.2f} T FMA/s, {100*fma/msH/1e9/19.7:.0f}% of the LDS bound), '
          f'torch conv2d {msHt*1e3:.1f} us;  data term {msD*1e3:.1f} us ({2*fma/msD/1e9:.2f} T FMA/s, '
          f'{100*2*fma/msD/1e9/19.7:.0f}%), torch autograd {msDt*1e3:.1f} us;  data term + last VJP {msV*1e3:.1f} us')
# sparse linear operators (operators.SparseLinear): ct32 = sparse-view parallel-beam CT, 32 views, m = 11 744 rows,
# 4 193 792 entries.  10 warm-up calls, then 100 timed ones between two events.  Yardstick in the same process:
# torch.sparse.mm on the CSR tensor over the plane-minor operand [n, P] (handed to it ready-made: it pays no transposes)
# and autograd for the gradient; if this torch build does not serve that on the device, the dense product at 64 x 64.
# Row reads of one product pass: nnz rows of 4 P bytes, against the 8.6 TB/s measured for index-gathered ~1 KiB rows.
def timeit100(f):
    for _ in range(10): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(100): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 100
oct = operators.build_operator('ct32', 3, 256, dev)
Pn = B * 3
nnz = oct.csr()[2].numel()
yc = K.randn_philox((B, oct.M), 1, 0, 4)
msH, msHt = timeit100(lambda: oct.H(x)), timeit100(lambda: oct.Ht(yc))
msD = timeit100(lambda: oct.data_term(x, yc, True))
msV = timeit100(lambda: oct.fused_last_vjp(x, e6, at, an, yc, g_e_out=ge, xt_next=cur))
gather = nnz * 4 * Pn
print(f'ct32 (m = {oct.m}, nnz = {nnz}) B={B}: H {msH*1e3:.1f} us, Ht {msHt*1e3:.1f} us, data term {msD*1e3:.1f} us, '
      f'data term + last VJP {msV*1e3:.1f} us;  row reads {gather/1e9:.2f} GB per product: two products over '
      f'the whole time of the data term = {2*gather/msD/1e9:.2f} TB/s of row reads (gather figure: 8.6 TB/s)')
try:
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        Acsr = operators.radon_matrix(256, 32).to(dev)
    xm = x.reshape(Pn, -1).t().contiguous()                      # [n, P]
    ym = yc.reshape(Pn, -1).t().contiguous()                     # [m, P]
    def torch_H():
        return torch.sparse.mm(Acsr, xm)
    def torch_data():
        xl = xm.detach().requires_grad_(True)
        loss = ((ym - torch.sparse.mm(Acsr, xl.clamp(-1, 1))) ** 2).sum()
        return torch.autograd.grad(loss, xl)
    tH, tD = timeit100(torch_H), timeit100(torch_data)
    print(f'    torch.sparse.mm CSR [n, P] B={B}: H {tH*1e3:.1f} us ({tH/msH:.2f} x ours), data term by autograd {tD*1e3:.1f} us '
          f'({tD/msD:.2f} x ours)')
except Exception as exc:                                         # say so, and measure the dense product at 64 x 64 instead
    print(f'    torch.sparse.mm on a CSR tensor with autograd is not served on this device: {type(exc).__name__}: {exc}')
    o64 = operators.build_operator('ct32', 3, 64, dev)
    x64, y64 = torch.randn(B, 3, 64, 64, device=dev), torch.randn(B, o64.M, device=dev)
    A64 = operators.radon_matrix(64, 32).to_dense().to(dev)
    def dense_data():
        xl = x64.reshape(Pn, -1).detach().requires_grad_(True)
        loss = ((y64.reshape(Pn, -1) - xl.clamp(-1, 1) @ A64.t()) ** 2).sum()
        return torch.autograd.grad(loss, xl)
    m64, t64 = timeit100(lambda: o64.data_term(x64, y64, True)), timeit100(dense_data)
    print(f'    ct32 at 64 x 64 B={B}: data term {m64*1e3:.1f} us, torch dense product + autograd {t64*1e3:.1f} us ({t64/m64:.2f} x ours)')
fourier_leg()
modfourier_leg()
