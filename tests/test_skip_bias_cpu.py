"""CPU: the skip-bias entry of the eight-wave Winograd kernel (nhmc_conv3x3_wino_skip) validates its arguments before any
device work, in the order of nhmc_conv3x3_wino, with fake aligned and unaligned pointers in the style of
tests/test_wino_shapes_cpu.py; its coverage query follows NHMC_WINO_WAVES and, in Python, NHMC_SKIP_BIAS."""


def test_entry_refuses_what_it_does_not_cover(monkeypatch):
    import ctypes
    import nhmc
    import nhmc.kernels as K
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    a, b, c, d, e, null = P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x5000), P(0)
    call = lambda x=a, u=b, add=d, ab=e, y=c, w=64, k=64: lib.nhmc_conv3x3_wino_skip(x, u, null, add, ab, y, 1, 8, k, 4, w, None)
    assert call(add=null) == 1 and call(ab=null) == 1 and call(x=null) == 1 and call(y=a) == 1 and call(add=a) == 1
    assert call(w=32) == 3 and call(k=32) == 3                                      # the wide geometry, K % 64 == 0
    assert call(add=P(0x4004)) == 2 and call(y=P(0x3004)) == 2
    assert call(add=null, w=32, y=P(0x3004)) == 1 and call(w=32, y=P(0x3004)) == 3   # ARG, SHAPE, ALIGN
    monkeypatch.setenv('NHMC_WINO_WAVES', '4')
    assert call() == 3 and not K.conv3x3_wino_skip_covers(1, 8, 64, 4, 64)
    monkeypatch.delenv('NHMC_WINO_WAVES')
    monkeypatch.setenv('NHMC_SKIP_BIAS', '0')
    assert not K.conv3x3_wino_skip_covers(1, 8, 64, 4, 64)
    assert nhmc._lib.load().nhmc_abi_version() == 2
