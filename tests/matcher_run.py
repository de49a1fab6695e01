"""One batch through jn_sgm_* / jn_bm_* (the C ABI, through the package's ctypes mirror) for the GPU tests of the two modes and of the matcher matrix."""
import numpy as np

LEFT_POISON, RIGHT_POISON = 199, 7            # what the caller's padding holds: never pixels


def run(jn, Matcher, p, Ls, Rs, pad=0, gap=0, extra=0, smaller_first=False):
    """Ls, Rs [n][H][W] uint8 -> (int16 maps [n][H][W], u8 maps, the handle's stage times).  Matcher: jn.Sgm or jn.Bm.
    pad: pitch = W + pad; gap: rows between two images (image_stride = (H + gap) pitch); padding and gap bytes are poisoned.
    extra: max_batch = n + extra.  smaller_first: frames 1 .. n-1 go through the handle as a batch of n - 1 first and must come out the same
    inside the batch of n (the handle's buffers are reused)."""
    from jackal_navigation_amd.device import DeviceArray
    n, H, W = Ls.shape
    pitch, rows = W + pad, H + gap
    Lp = np.full((n, rows, pitch), LEFT_POISON, np.uint8); Rp = np.full((n, rows, pitch), RIGHT_POISON, np.uint8)
    Lp[:, :H, :W] = Ls; Rp[:, :H, :W] = Rs
    dL, dR = DeviceArray.from_numpy(Lp), DeviceArray.from_numpy(Rp)
    dD = DeviceArray((n, H, W), np.int16)
    with Matcher(p, W, H, max_batch=n + extra) as s:
        first = None
        if smaller_first and n > 1:
            s.process_batch(n - 1, dL.ptr + rows * pitch, dR.ptr + rows * pitch, pitch, rows * pitch, dD.ptr)
            first = dD.numpy()[:n - 1].copy()
        s.process_batch(n, dL.ptr, dR.ptr, pitch, rows * pitch, dD.ptr)
        t = s.last_times()
        du8 = DeviceArray((n, H, W), np.uint8)
        s.to_u8(dD.ptr, du8.ptr, n * H * W)
    out, u8 = dD.numpy(), du8.numpy()
    for a in (dL, dR, dD, du8):
        a.free()
    if first is not None:
        assert np.array_equal(first, out[1:]), "a batch of %d and the same frames inside a batch of %d give different maps" % (n - 1, n)
    return out, u8, t
