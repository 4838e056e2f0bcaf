"""ADVENT's discriminator convolution (4x4 / stride 2 / pad 1, LeakyReLU in front) on the pre-split conv kernels: the weight
packer of the space-to-depth form, the two rearrangement launches (csrc/disc.hip) and the autograd function around them."""
import torch

from .._lib import call
from . import _state
from . import conv as _conv
from .core import _desc, _p, _require_cuda, _stream, as_nhwc, nhwc_ld
from .limbs import Limbs, amax_slot, is_limb_only, known_amax, limb_only, tag_amax


def _up32(n):
    return -(-n // 32) * 32


def s2d_weight(weight, cout_pad):
    """OIHW [Cout,C,4,4] -> the 2x2 weight over the space-to-depth channels, [cout_pad, Cp, 2, 2] with
    w2[o, (py*2+px)*C + c, a, b] = w[o, c, 2a+py, 2b+px]; rows Cout.. and channels 4C..Cp are zero."""
    cout, C, kh, kw = weight.shape
    w2 = torch.zeros(cout_pad, _up32(4 * C), 2, 2, device=weight.device, dtype=torch.float32)
    w2[:cout, :4 * C] = weight.detach().reshape(cout, C, 2, 2, 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(cout, 4 * C, 2, 2)
    return w2


def s2d_weight_grad(dw2, cout, C):
    """The way back for the gradient: [>=Cout, >=4C, 2, 2] -> OIHW [Cout,C,4,4]."""
    return dw2[:cout, :4 * C].reshape(cout, 2, 2, C, 2, 2).permute(0, 3, 4, 1, 5, 2).reshape(cout, C, 4, 4)


class DiscPackCache(_conv._PackCache):
    """_PackCache for a discriminator conv: the rearranged weight is built once per parameter version, its forward and its
    data-gradient packing are made from it when first asked for (the adversarial pass never asks for the weight gradient's
    side, the discriminator pass's layer 0 never for the data gradient's) and share its max|w|."""

    def __init__(self):
        super().__init__()
        self.key_w = self.w2 = None

    def _w2(self, w, key):
        if self.key_w != key:
            self.w2, self.key_w = s2d_weight(w, _up32(w.shape[0])), key
        return self.w2

    def get_fwd(self, w, cout_pad=None, kp=None):
        k = self._key(w)
        if self.key_f != k:
            w2 = self._w2(w, k)
            self.fwd, self.key_f = _conv._pack_h2(w2, w2.shape[0], 4 * w2.shape[1], 0, w2.shape[0]), k
        return self.fwd

    def get_dgrad(self, w, cout_pad=None):
        k = self._key(w)
        if self.key_d != k:
            w2 = self._w2(w, k)
            self.dgrad, self.key_d = _conv._pack_h2(w2, w2.shape[1], 4 * w2.shape[0], 1, w2.shape[0]), k
        return self.dgrad

    def __deepcopy__(self, memo):
        return DiscPackCache()


def s2d_split(x, nchw, slope):
    """Limb rows of the space-to-depth view of LeakyReLU(x) under a one-pixel zero border, as a limb-only [B,Hs,Ws,Cp]
    activation.  x: fp32 [B,C,H,W] (nchw) or an NHWC view.  The scale is max|x| (a bound on max|S|)."""
    if nchw:
        x = x.contiguous()
        B, C, H, W = x.shape
        ldx = 0
    else:
        x = as_nhwc(x)
        B, H, W, C = x.shape
        ldx = nhwc_ld(x)
    amax = known_amax(x)
    if amax is None:
        amax = amax_slot(x.device)
        if nchw:
            call("onda_absmax", _p(x), 1, x.numel(), x.numel(), _p(amax), _stream())
        else:
            call("onda_absmax", _p(x), B * H * W, C, ldx, _p(amax), _stream())
        tag_amax(x, amax)
    Hs, Ws, Cp = H // 2 + 1, W // 2 + 1, _up32(4 * C)
    rows = B * Hs * Ws
    planes = torch.empty(rows, 2 * Cp, device=x.device, dtype=torch.float16)
    call("onda_s2d_split_h2", _p(x), int(nchw), B, C, H, W, ldx, float(slope), _p(amax), _p(planes), _stream())
    return x, limb_only((B, Hs, Ws, Cp), x.device, Limbs(planes, amax, Cp, rows * Cp))


def d2s_bwd(gs, gamax, x, nchw, shape, slope, want_f32):
    """Gradient of x from the fp32 gradient `gs` of its space-to-depth view (max|gs| in `gamax`).  nchw: fp32 [B,C,H,W].
    Otherwise NHWC limb rows scaled by the bound max|gs| -- limb-only, or, with `want_f32`, an fp32 tensor that carries them."""
    B, C, H, W = shape
    dev = gs.device
    if nchw:
        dx = torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
        call("onda_d2s_bwd", _p(gs), None, _p(x), 1, B, C, H, W, 0, float(slope), None, _p(dx), _stream())
        return dx
    planes = torch.empty(B * H * W, 2 * C, device=dev, dtype=torch.float16)
    lb = Limbs(planes, gamax, C, B * H * W * C)
    dx = torch.empty(B, H, W, C, device=dev, dtype=torch.float32) if want_f32 else None
    call("onda_d2s_bwd", _p(gs), _p(gamax), _p(x), 0, B, C, H, W, nhwc_ld(x) if x is not None else 0, float(slope), _p(planes),
         _p(dx), _stream())
    if dx is None:
        return limb_only((B, H, W, C), dev, lb)
    dx._onda_limbs = (dx._version, lb)
    return dx


class DiscConvFn(torch.autograd.Function):
    """y[B,Ho,Wo,Cout up to 32] = conv4x4/2/1(LeakyReLU(x)) + bias on the pre-split kernels (module docstring, csrc/disc.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, cache, slope, nchw, grad_f32):
        _require_cuda(x, "discriminator conv input")
        if _state.CONV_MODE != "f16x2" or _state.H2_PATH != "dma":
            raise RuntimeError("onda_amd: the discriminator conv runs on the pre-split \"f16x2\" kernels only")
        cout, C, kh, kw = weight.shape
        if (kh, kw) != (4, 4) or x.dim() != 4 or x.dtype != torch.float32 or x.shape[1 if nchw else 3] != C:
            raise RuntimeError("onda_amd: disc_conv takes an fp32 4-D input and a [Cout,C,4,4] weight")
        if not nchw and C % 32 != 0:
            raise RuntimeError("onda_amd: an NHWC discriminator conv input needs a multiple of 32 channels")
        x, S = s2d_split(x, nchw, slope)
        B, Hs, Ws, Cp = S.shape
        co = _up32(cout)
        sl = S._onda_limbs[1]
        y = torch.empty(B, Hs - 1, Ws - 1, co, device=x.device, dtype=torch.float32)
        yamax = amax_slot(x.device)
        d = _desc(B, Hs, Ws, Cp, Hs - 1, Ws - 1, co, 2, 1, 1, 0, Cp, co)
        _conv._launch_l2("fwd", sl, cache.get_fwd(weight), y, d, shift=_conv._pad_vec(bias, co), yamax=yamax,
                         tag_dims=(B * (Hs - 1) * (Ws - 1), co, Cp, 2, 1, 1))
        tag_amax(y, yamax)  # the next layer's scale: no max pass over y
        mask = x if (slope != 1.0 and ctx.needs_input_grad[0]) else None  # fp32 input: kept for the LeakyReLU derivative only
        ctx.save_for_backward(mask, weight)
        ctx.S = S if ctx.needs_input_grad[1] else None  # the operand the weight gradient reads, kept once, as limb rows
        ctx.cache, ctx.geom, ctx.has_bias = cache, (tuple(x.shape), cout, C, Cp, Hs, Ws, co, slope, nchw, grad_f32), bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        mask, weight = ctx.saved_tensors
        xshape, cout, C, Cp, Hs, Ws, co, slope, nchw, grad_f32 = ctx.geom
        if not is_limb_only(dy):
            dy = as_nhwc(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            gamax = amax_slot(dy.device)
            gs = _conv.conv_dgrad(dy, ctx.cache.get_dgrad(weight), 2, 1, 1, 0, Cp, (Hs, Ws), yamax=gamax)
            shape = xshape if nchw else (xshape[0], xshape[3], xshape[1], xshape[2])
            dx = d2s_bwd(gs, gamax, mask, nchw, shape, slope, grad_f32)
        if ctx.needs_input_grad[1]:
            dw2 = _conv.conv_wgrad(ctx.S, dy, 2, 1, 1, 0, co, Cp, xlimbs=ctx.S._onda_limbs[1])
            dw = s2d_weight_grad(dw2, cout, C)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            if is_limb_only(dy):
                raise RuntimeError("onda_amd: the bias gradient of a discriminator conv needs the fp32 output gradient "
                                   "(the layer above was built with grad_f32=False)")
            db = _conv.colsum(dy)[:cout]
        return dx, dw, db, None, None, None, None


def disc_conv(x, weight, bias, slope_in=1.0, cache=None, nchw=False, grad_f32=True):
    """conv 4x4 / stride 2 / pad 1 of LeakyReLU(x, slope_in) (slope_in = 1: no activation) + bias, NHWC [B,H//2,W//2,Cout] out.
    x: fp32 NHWC view with C % 32 == 0 channels, or (nchw) a [B,C,H,W] tensor of any C.  Backward computes what
    needs_input_grad asks for and nothing else: the data gradient (2x2 stride-1 data gradient + onda_d2s_bwd), the weight
    gradient (onda_conv2d_wgrad_l2 over the kept limb rows), the bias gradient (colsum).
    grad_f32: hand the gradient of an NHWC x on as an fp32 tensor that carries its limb rows (what a producer with a bias
    gradient needs); False: as limb rows only."""
    cache = cache if cache is not None else DiscPackCache()
    y = DiscConvFn.apply(x, weight, bias, cache, float(slope_in), bool(nchw), bool(grad_f32))
    return y if y.shape[3] == weight.shape[0] else y[..., :weight.shape[0]]
