"""The argument surface of the six loss entry points (lograst_loss_forward / _backward, their _gain and _masked forms;
log_amd/csrc/api.hip), pinned as a literal table: (entry point, one fault) -> return code and a fragment of the message.
Every row fails a check before any device work, so the pointers are never dereferenced and the table runs without a GPU.

The scratch check is the last one before the launch, so "one byte under the threshold" is a row of the table and "exactly
at the threshold" needs real buffers: test_scratch_exactly_at_the_threshold_is_accepted, the only test here that is
marked gpu.  Shape 4 x 3 x 42 x 42 throughout: 12 forward workgroups (one 32 x 32 tile of the 32 x 32 outputs per plane) but
48 backward workgroups (2 x 2 image tiles per plane), so the three sizing functions give 256, 512 and 512 bytes and the
smaller size lograst_loss_forward_gain accepts is distinguishable from the one its message names."""
import ctypes

import pytest
import torch

OK, ERR_ARG = 0, -1
B, C, H, W = 4, 3, 42, 42
P, Q = 0x1000, 0x2000                                        # never dereferenced


def s4(*v):
    return (ctypes.c_int64 * 4)(*v)


def s3(*v):
    return (ctypes.c_int64 * 3)(*v)


S4, S3 = s4(C * H * W, H * W, W, 1), s3(H * W, W, 1)
BIG = 1 << 20

# per entry point: the parameters in the order of the C signature, and a call that passes every check
ORDER = {
    "forward": "B C H W render rs render_l1 ls gt gs ssim_weight l1_weight out3 maps scratch nbytes stream",
    "backward": "B C H W render rs render_l1 ls gt gs l1_weight grad_loss maps grad_render grad_render_l1 stream",
    "forward_gain": "B C H W render rs gt gs l1_gain ssim_weight l1_weight out3 maps scratch nbytes stream",
    "backward_gain": "B C H W render rs gt gs l1_gain l1_weight grad_loss maps grad_render grad_gain scratch nbytes stream",
    "forward_masked": "B C H W render rs render_l1 ls gt gs l1_gain mask ms foreground fs background gt_out ssim_weight "
                      "l1_weight out3 maps scratch nbytes stream",
    "backward_masked": "B C H W render rs render_l1 ls gt gs l1_gain mask ms l1_weight grad_loss maps grad_render "
                       "grad_render_l1 grad_gain scratch nbytes stream",
}
GOOD = dict(B=B, C=C, H=H, W=W, render=P, rs=S4, render_l1=None, ls=None, gt=P, gs=S4, ssim_weight=0.2, l1_weight=0.8, out3=P,
            maps=P, scratch=P, nbytes=BIG, stream=None, grad_loss=P, grad_render=P, grad_render_l1=None, l1_gain=None,
            grad_gain=None, mask=None, ms=None, foreground=None, fs=None, background=None, gt_out=None)
GOOD_OF = {
    "forward": {}, "backward": {},
    "forward_gain": dict(l1_gain=P), "backward_gain": dict(l1_gain=P, grad_gain=P),
    "forward_masked": dict(mask=P, ms=S3), "backward_masked": dict(mask=P, ms=S3),
}
ALL = tuple(ORDER)
FORWARDS = ("forward", "forward_gain", "forward_masked")
BACKWARDS = ("backward", "backward_gain", "backward_masked")
WITH_L1 = ("forward", "backward", "forward_masked", "backward_masked")          # the entry points with a render_l1
MASKED = ("forward_masked", "backward_masked")

WINDOW = b"image smaller than the 11-pixel window of the SSIM (height and width must be >= 11)"
STRIDES = b"y / x strides reach beyond 2^31 - 1 elements inside one image plane"
EXCLUSIVE = b"render_l1 and l1_gain are mutually exclusive: the L1 term reads one of them"
NO_GRAD_L1 = b"render_l1 is a tensor of its own but grad_render_l1 is NULL"
SCRATCH = b"loss scratch too small (%s) or not 8-byte aligned"
SCRATCH_PLAIN, SCRATCH_GAIN, SCRATCH_MASKED = (SCRATCH % n for n in (
    b"lograst_loss_scratch_bytes", b"lograst_loss_gain_scratch_bytes", b"lograst_loss_masked_scratch_bytes"))
OVER = 2 ** 31                                               # one past the largest in-plane offset
ROW_OVER = 52377650                                          # 41 * ROW_OVER = 2^31 + 2: each stride fits, their reach does not
GAIN_ARGS = dict(l1_gain=P, grad_gain=P)

# (entry points, the fault, what the row changes in the good call, return code, message fragment or None)
TABLE = [
    # ---- geometry (lr_loss_args), every entry point
    (ALL, "negative batch", dict(B=-1), ERR_ARG, b"negative batch or channel count"),
    (ALL, "negative channels", dict(C=-1), ERR_ARG, b"negative batch or channel count"),
    (ALL, "height 10", dict(H=10), ERR_ARG, WINDOW),
    (ALL, "width 10", dict(W=10), ERR_ARG, WINDOW),
    (ALL, "empty batch, width 10", dict(B=0, W=10), ERR_ARG, WINDOW),
    (ALL, "2^31 elements", dict(B=1, H=32768, W=21846), ERR_ARG, b"more than 2^31 - 1 image elements"),
    # ---- NULL images and strides
    (ALL, "render NULL", dict(render=None), ERR_ARG, b"NULL pointer"),
    (ALL, "gt NULL", dict(gt=None), ERR_ARG, b"NULL pointer"),
    (ALL, "render strides NULL", dict(rs=None), ERR_ARG, b"NULL pointer"),
    (ALL, "gt strides NULL", dict(gs=None), ERR_ARG, b"NULL pointer"),
    (WITH_L1, "render_l1 without strides", dict(render_l1=Q, grad_render_l1=P), ERR_ARG, b"NULL pointer"),
    # ---- the 32-bit offsets inside a plane: image strides
    (ALL, "render stride y", dict(rs=s4(0, 0, OVER, 1)), ERR_ARG, STRIDES),
    (ALL, "render stride y negative", dict(rs=s4(0, 0, -OVER, 1)), ERR_ARG, STRIDES),
    (ALL, "render stride x", dict(rs=s4(0, 0, 1, OVER)), ERR_ARG, STRIDES),
    (ALL, "render reach", dict(rs=s4(0, 0, ROW_OVER, 0)), ERR_ARG, STRIDES),
    (ALL, "gt stride y", dict(gs=s4(0, 0, OVER, 1)), ERR_ARG, STRIDES),
    (ALL, "gt reach", dict(gs=s4(0, 0, 1, ROW_OVER)), ERR_ARG, STRIDES),
    (WITH_L1, "render_l1 stride x", dict(render_l1=Q, ls=s4(0, 0, 1, -OVER), grad_render_l1=P), ERR_ARG, STRIDES),
    (WITH_L1, "render_l1 reach", dict(render_l1=Q, ls=s4(0, 0, ROW_OVER, 0), grad_render_l1=P), ERR_ARG, STRIDES),
    # ... what is no fault goes on to the next check: negative strides count by magnitude, batch and channel strides are
    # free, and the strides of an absent render_l1 are not read
    (FORWARDS, "negative strides in range, out3 NULL", dict(rs=s4(-2 ** 40, 2 ** 40, -W, -1), out3=None), ERR_ARG, b"out3 is NULL"),
    (("forward", "forward_masked"), "strides of no render_l1, out3 NULL", dict(ls=s4(0, 0, OVER, OVER), out3=None), ERR_ARG,
     b"out3 is NULL"),
    # ---- forwards
    (FORWARDS, "out3 NULL", dict(out3=None), ERR_ARG, b"out3 is NULL"),
    (FORWARDS, "empty batch, out3 NULL", dict(B=0, out3=None), ERR_ARG, b"out3 is NULL"),
    (FORWARDS, "no channels, out3 NULL", dict(C=0, out3=None), ERR_ARG, b"out3 is NULL"),
    (("forward_gain",), "l1_gain NULL", dict(l1_gain=None), ERR_ARG, b"l1_gain is NULL"),
    # ---- backwards: the empty batch returns before the pointers are looked at
    (BACKWARDS, "empty batch, everything NULL", dict(B=0, render=None, rs=None, gt=None, gs=None, grad_loss=None, maps=None,
                                                      grad_render=None, l1_gain=None, grad_gain=None, scratch=None, nbytes=0), OK, None),
    (BACKWARDS, "no channels", dict(C=0, grad_loss=None, maps=None, grad_render=None, scratch=None, nbytes=0), OK, None),
    (BACKWARDS, "grad_loss NULL", dict(grad_loss=None), ERR_ARG, b"NULL pointer"),
    (BACKWARDS, "maps NULL", dict(maps=None), ERR_ARG, b"NULL pointer"),
    (BACKWARDS, "grad_render NULL", dict(grad_render=None), ERR_ARG, b"NULL pointer"),
    (("backward", "backward_masked"), "render_l1 of its own, grad_render_l1 NULL", dict(render_l1=Q, ls=S4), ERR_ARG, NO_GRAD_L1),
    (("backward", "backward_masked"), "render_l1 at render with other strides, grad_render_l1 NULL",
     dict(render_l1=P, ls=s4(C * H * W, H * W, 1, H)), ERR_ARG, NO_GRAD_L1),
    (("backward_gain",), "l1_gain NULL", dict(l1_gain=None), ERR_ARG, b"NULL pointer"),
    (("backward_gain",), "grad_gain NULL", dict(grad_gain=None), ERR_ARG, b"NULL pointer"),
    (("backward_masked",), "l1_gain without grad_gain", dict(l1_gain=P), ERR_ARG, b"NULL pointer"),
    # ... render_l1 == render through the same strides is no tensor of its own: the call goes on to the next check
    (("backward_masked",), "render_l1 is render, grad_render_l1 NULL, mask strides NULL", dict(render_l1=P, ls=S4, ms=None), ERR_ARG,
     b"mask without strides"),
    # ---- the masked pair: exclusivity and the NULL preconditions
    (MASKED, "render_l1 and l1_gain", dict(render_l1=Q, ls=S4, grad_render_l1=P, **GAIN_ARGS), ERR_ARG, EXCLUSIVE),
    (MASKED, "empty batch, render_l1 and l1_gain", dict(B=0, render_l1=Q, ls=S4, grad_render_l1=P, **GAIN_ARGS), ERR_ARG, EXCLUSIVE),
    (("forward_masked",), "mask and foreground NULL", dict(mask=None, ms=None), ERR_ARG,
     b"mask and foreground are both NULL: use lograst_loss_forward / _gain"),
    (("forward_masked",), "empty batch, mask and foreground NULL", dict(B=0, mask=None, ms=None), ERR_ARG,
     b"mask and foreground are both NULL: use lograst_loss_forward / _gain"),
    (("forward_masked",), "foreground without background", dict(foreground=P, fs=S3, gt_out=P), ERR_ARG,
     b"foreground needs background and gt_out"),
    (("forward_masked",), "foreground without gt_out", dict(foreground=P, fs=S3, background=P), ERR_ARG,
     b"foreground needs background and gt_out"),
    (("forward_masked",), "foreground alone without gt_out", dict(mask=None, ms=None, foreground=P, fs=S3, background=P), ERR_ARG,
     b"foreground needs background and gt_out"),
    (("backward_masked",), "mask NULL", dict(mask=None, ms=None), ERR_ARG,
     b"mask is NULL: use lograst_loss_backward / _gain on the composited gt"),
    (("backward_masked",), "empty batch, mask NULL", dict(B=0, mask=None, ms=None), ERR_ARG,
     b"mask is NULL: use lograst_loss_backward / _gain on the composited gt"),
    (MASKED, "mask without strides", dict(ms=None), ERR_ARG, b"mask without strides"),
    (("forward_masked",), "foreground without strides", dict(foreground=P, background=P, gt_out=P), ERR_ARG,
     b"foreground without strides"),
    # ---- the 32-bit offsets inside a plane: mask and foreground strides
    (MASKED, "mask stride y", dict(ms=s3(0, OVER, 1)), ERR_ARG, STRIDES),
    (MASKED, "mask stride x negative", dict(ms=s3(0, 1, -OVER)), ERR_ARG, STRIDES),
    (MASKED, "mask reach", dict(ms=s3(0, ROW_OVER, 0)), ERR_ARG, STRIDES),
    (("forward_masked",), "foreground stride y", dict(foreground=P, fs=s3(0, -OVER, 1), background=P, gt_out=P), ERR_ARG, STRIDES),
    (("forward_masked",), "foreground stride x", dict(foreground=P, fs=s3(0, 1, OVER), background=P, gt_out=P), ERR_ARG, STRIDES),
    (("forward_masked",), "foreground reach", dict(mask=None, ms=None, foreground=P, fs=s3(2 ** 40, 0, ROW_OVER), background=P,
                                                   gt_out=P), ERR_ARG, STRIDES),
    # ---- scratch: NULL, one byte under the size the entry point accepts, misaligned; each with its own sizing-function name
    (("forward",), "scratch NULL", dict(scratch=None), ERR_ARG, SCRATCH_PLAIN),
    (("forward",), "scratch 255 bytes", dict(nbytes=255), ERR_ARG, SCRATCH_PLAIN),
    (("forward",), "scratch misaligned", dict(scratch=P + 4), ERR_ARG, SCRATCH_PLAIN),
    (("forward_gain",), "scratch NULL", dict(scratch=None), ERR_ARG, SCRATCH_GAIN),
    (("forward_gain",), "scratch 255 bytes", dict(nbytes=255), ERR_ARG, SCRATCH_GAIN),     # (under lograst_loss_scratch_bytes)
    (("forward_gain",), "scratch misaligned", dict(scratch=P + 4), ERR_ARG, SCRATCH_GAIN),
    (("backward_gain",), "scratch NULL", dict(scratch=None), ERR_ARG, SCRATCH_GAIN),
    (("backward_gain",), "scratch 511 bytes", dict(nbytes=511), ERR_ARG, SCRATCH_GAIN),
    (("backward_gain",), "scratch of the forward's size", dict(nbytes=256), ERR_ARG, SCRATCH_GAIN),
    (("backward_gain",), "scratch misaligned", dict(scratch=P + 1), ERR_ARG, SCRATCH_GAIN),
    (("forward_masked",), "scratch NULL", dict(scratch=None), ERR_ARG, SCRATCH_MASKED),
    (("forward_masked",), "scratch 511 bytes", dict(nbytes=511), ERR_ARG, SCRATCH_MASKED),
    (("forward_masked",), "scratch misaligned", dict(scratch=P + 2), ERR_ARG, SCRATCH_MASKED),
    (("backward_masked",), "gain, scratch NULL", dict(scratch=None, **GAIN_ARGS), ERR_ARG, SCRATCH_MASKED),
    (("backward_masked",), "gain, scratch 511 bytes", dict(nbytes=511, **GAIN_ARGS), ERR_ARG, SCRATCH_MASKED),
    (("backward_masked",), "gain, scratch misaligned", dict(scratch=P + 4, **GAIN_ARGS), ERR_ARG, SCRATCH_MASKED),
]
ROWS = [(entry, fault, change, rc, words) for entries, fault, change, rc, words in TABLE for entry in entries]


def _call(L, entry, change):
    names = ORDER[entry].split()
    args = {**GOOD, **GOOD_OF[entry], **change}
    assert set(change) <= set(GOOD), change
    return getattr(L, "lograst_loss_" + entry)(*(args[n] for n in names))


def test_the_sizes_the_table_stands_on():
    from log_amd import _lib
    L = _lib.lib()
    assert L.lograst_loss_scratch_bytes(B, C, H, W) == 256
    assert L.lograst_loss_gain_scratch_bytes(B, C, H, W) == 512
    assert L.lograst_loss_masked_scratch_bytes(B, C, H, W) == 512
    assert 41 * (ROW_OVER - 1) <= 2 ** 31 - 1 < 41 * ROW_OVER and ROW_OVER < 2 ** 31 - 1
    assert {e for entries, *_ in TABLE for e in entries} == set(ALL)


@pytest.mark.parametrize("entry,fault,change,rc,words", ROWS, ids=[f"{r[0]}-{r[1]}".replace(" ", "_") for r in ROWS])
def test_one_fault_one_message(entry, fault, change, rc, words):
    from log_amd import _lib
    L = _lib.lib()
    got = _call(L, entry, change)
    assert got == rc, (got, L.lograst_last_error())
    if words is not None:
        assert words in L.lograst_last_error(), L.lograst_last_error()


@pytest.mark.gpu
def test_scratch_exactly_at_the_threshold_is_accepted():
    """The other side of the "one byte under" rows: each entry point runs with a scratch of exactly the size it accepts --
    lograst_loss_forward_gain with the 256 bytes of lograst_loss_scratch_bytes, not the 512 its message names."""
    from log_amd import _lib
    from log_amd.rasterizer import _ptr, _stream_ptr
    L = _lib.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    render, gt = (torch.rand(B, C, H, W, device=dev, generator=g) for _ in range(2))
    mask, gain = torch.rand(B, H, W, device=dev, generator=g), torch.rand(B, C, device=dev, generator=g) + 0.5
    out3, one = torch.empty(3, device=dev), torch.ones(1, device=dev)
    maps = torch.empty(3 * B * C * (H - 10) * (W - 10), device=dev)
    grad, grad_gain = torch.empty(B, C, H, W, device=dev), torch.zeros(B, C, device=dev)
    scratch = {n: torch.empty(n, dtype=torch.uint8, device=dev) for n in (256, 512)}
    real = dict(render=_ptr(render), rs=s4(*render.stride()), gt=_ptr(gt), gs=s4(*gt.stride()), out3=_ptr(out3), maps=_ptr(maps),
                grad_loss=_ptr(one), grad_render=_ptr(grad))
    with_gain = dict(l1_gain=_ptr(gain), grad_gain=_ptr(grad_gain))
    with_mask = dict(mask=_ptr(mask), ms=s3(*mask.stride()))
    with torch.cuda.device(dev):
        stream = _stream_ptr(dev)
        for entry, nbytes, more in (("forward", 256, {}), ("forward_gain", 256, with_gain), ("backward_gain", 512, with_gain),
                                    ("forward_masked", 512, {**with_mask, **with_gain}),
                                    ("backward_masked", 512, {**with_mask, **with_gain})):
            rc = _call(L, entry, {**real, **more, "scratch": _ptr(scratch[nbytes]), "nbytes": nbytes, "stream": stream})
            assert rc == OK, (entry, rc, L.lograst_last_error())
        torch.cuda.synchronize(dev)
    assert torch.isfinite(out3).all() and torch.isfinite(grad).all() and torch.isfinite(grad_gain).all()
