"""Reference, working-precision model and per-element error gate for the dense-block 3x3 convolution (csrc/upscaler.hip,
include/fluxmi.h fluxmi_conv3x3_dense) and for the RRDBNet built on it (modules/upscaler.py).  CPU only.

  conv_ref64     the convolution with its epilogue, and A = the same expression on absolute values, in fp64 on the bf16 values
  conv_model     the same in fp32 with the header's rounding points (two operations per scale-and-add, ONE bf16 rounding at the store) and
                 nothing else, in two tap orders; `mut` names one deliberate defect (MUTANTS) for the test that the gate can see it
  conv_gate      what conv_check needs, from the inputs alone
  conv_check     every element within MARGIN * (u |ref| + (9 Cin + 4) 2^-24 A)
  conv_inputs    the seeded input families the CPU mutation test and the GPU tests share
  net_ref64 / net_model   the whole network (BasicSR key layout) in fp64 without any rounding / in fp32 with a bf16 rounding per launch

The bound: u = 2^-8 is the bf16 unit roundoff, u |ref| the rounding of the store; an fp32 sum of 9 Cin products plus the at most four
epilogue operations is off by at most (9 Cin + 4) 2^-24 times the sum of the absolute values, which is A.  MARGIN = 1.25
(attention_ref.MARGIN) is what separates first-order bounds from the real thing.  Nothing here is measured on the kernel.

Tensors are NHWC: x [B, Hi, Wi, C], w [Cout, 3, 3, Cin], bias [Cout], residuals [B, H, W, Cout]; (H, W) = upsample * (Hi, Wi).
"""
import torch
import torch.nn.functional as F

from attention_ref import MARGIN, U_BF16, _rel_l2, _worst_ratio

TILE = 16  # the kernel's pixel tile edge (include/fluxmi.h FLUXMI_CONV_DENSE_TILE)
FAMILIES = ("randn", "neg", "probe")
MUTANTS = ("slope", "drop_tap", "wrap_w", "no_res_scale", "up_offset", "chan_shift", "batch_leak")
SHIFT = 16  # chan_shift reads the window this many channels off; conv_inputs' x buffer is that much wider than Cin
ARMS_NONE = dict(bias=False, act=False, r1=False, r2=False, upsample=1)
# the epilogue arms under which a mutant differs from the model at all (slope needs act, no_res_scale a residual, up_offset the upsample);
# slope is judged without residuals: behind a1 * a2 = 0.04 and two O(1) residuals its 25 % change of the negative half would hide in u |ref|
MUTANT_ARMS = {
    "slope": dict(bias=True, act=True, r1=False, r2=False, upsample=1),
    "drop_tap": dict(bias=True, act=True, r1=True, r2=True, upsample=1),
    "wrap_w": dict(bias=True, act=True, r1=True, r2=True, upsample=1),
    "no_res_scale": dict(bias=True, act=True, r1=True, r2=True, upsample=1),
    "up_offset": dict(bias=True, act=True, r1=False, r2=False, upsample=2),
    "chan_shift": dict(bias=True, act=True, r1=True, r2=True, upsample=1),
    "batch_leak": dict(bias=True, act=True, r1=True, r2=True, upsample=1),
}
A1, A2, SLOPE = 0.2, 0.2, 0.2


def _gather(x, upsample, mut=None):
    """nearest 2x upsample as the kernel's gather does it: output (y, x) <- input (y / 2, x / 2)"""
    if upsample == 1:
        return x
    Hi, Wi = x.shape[1], x.shape[2]
    off = 1 if mut == "up_offset" else 0
    iy = ((torch.arange(2 * Hi) + off) // 2).clamp(max=Hi - 1)
    ix = ((torch.arange(2 * Wi) + off) // 2).clamp(max=Wi - 1)
    return x[:, iy][:, :, ix]


def _padded(xu, mut=None):
    B, H, W, _ = xu.shape
    xp = F.pad(xu, (0, 0, 1, 1, 1, 1))
    if mut == "wrap_w":  # the right neighbour of column W - 1 comes from the next row's first column
        xp[:, 0:H, W + 1] = xu[:, 0:H, 0]
    if mut == "batch_leak" and B > 1:  # the bottom halo of image b is the top row of image b + 1
        xp[:-1, H + 1, 1 : W + 1] = xu[1:, 0]
    return xp


def _taps(xp, w, order=0, drop=None):
    """sum over taps of xp[.., y + dy, x + dx, :] @ w[:, dy, dx, :]^T in xp's dtype; order 0 walks (dy, dx) up, 1 down"""
    B, Hp, Wp, _ = xp.shape
    H, W = Hp - 2, Wp - 2
    acc = torch.zeros(B, H, W, w.shape[0], dtype=xp.dtype)
    taps = [(dy, dx) for dy in range(3) for dx in range(3)]
    for dy, dx in taps if order == 0 else reversed(taps):
        if (dy, dx) == drop:
            continue
        acc = acc + xp[:, dy : dy + H, dx : dx + W] @ w[:, dy, dx, :].T
    return acc


def _conv(x, w, bias, r1, a1, r2, a2, slope, act, upsample, dtype, order=0, mut=None, absolute=False):
    f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    y = _taps(_padded(_gather(f(x), upsample, mut), mut), f(w), order, (2, 2) if mut == "drop_tap" else None)
    if bias is not None:
        y = y + f(bias)
    if act and not absolute:
        s = torch.tensor(0.25 if mut == "slope" else slope, dtype=torch.float32).to(dtype)  # the kernel's slope is an fp32 value
        y = torch.where(y < 0, s * y, y)
    for r, a in ((r1, a1), (r2, a2)):
        if r is not None:
            a = torch.tensor(1.0 if mut == "no_res_scale" else a, dtype=torch.float32).to(dtype)  # the kernel's a is an fp32 value
            y = (a.abs() if absolute else a) * y + f(r)  # two rounded operations in fp32, as the header states
    return y


def conv_ref64(x, w, bias=None, r1=None, a1=1.0, r2=None, a2=1.0, slope=SLOPE, act=False, upsample=1):
    """(ref, A) in fp64"""
    args = (x, w, bias, r1, a1, r2, a2, slope, act, upsample, torch.float64)
    return _conv(*args), _conv(*args, absolute=True)


def conv_model(x, w, bias=None, r1=None, a1=1.0, r2=None, a2=1.0, slope=SLOPE, act=False, upsample=1, order=0, mut=None):
    """bf16 [B, H, W, Cout]: fp32 throughout, rounded once.  x holds the window's channels [0, Cin) first; chan_shift needs SHIFT more."""
    assert mut is None or mut in MUTANTS
    cin = w.shape[-1]
    xw = x[..., SHIFT : SHIFT + cin] if mut == "chan_shift" else x[..., :cin]
    return _conv(xw, w, bias, r1, a1, r2, a2, slope, act, upsample, torch.float32, order, mut).bfloat16()


def conv_inputs(family, B, Hi, Wi, Cin, Cout, seed, upsample=1):
    """Seeded bf16 tensors: xbuf [B, Hi, Wi, Cin + SHIFT] (the convolution reads the window [0, Cin)), w [Cout, 3, 3, Cin], bias [Cout],
    r1, r2 [B, H, W, Cout].
      randn   unit normal x, bias, residuals; w normal with variance 1 / (9 Cin): outputs O(1) with full cancellation
      neg     x >= 0, w <= 0, bias <= 0: every pre-activation is negative (the slope acts everywhere) and nothing cancels, so A = |ref|
              before the residuals: the tightest bound
      probe   w one-hot: output channel co copies +-x at tap co % 9, input channel (5 co + 3) % Cin -- every tap and window edge by itself"""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed * 1000003 + FAMILIES.index(family) * 7919 + Cin * 131 + Cout * 17 + Hi * 5 + Wi)
    rn = lambda *s: torch.randn(*s, generator=g)
    H, W = Hi * upsample, Wi * upsample
    xbuf, w, bias = rn(B, Hi, Wi, Cin + SHIFT), rn(Cout, 3, 3, Cin) / (9 * Cin) ** 0.5, rn(Cout)
    r1, r2 = rn(B, H, W, Cout), rn(B, H, W, Cout)
    if family == "neg":
        xbuf, w, bias = xbuf.abs(), -w.abs(), -bias.abs()
    elif family == "probe":
        w = torch.zeros(Cout, 3, 3, Cin)
        co = torch.arange(Cout)
        sign = torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0)
        w[co, (co % 9) // 3, (co % 9) % 3, (5 * co + 3) % Cin] = sign
        bias = 0.25 * bias
    return dict(xbuf=xbuf.bfloat16(), w=w.bfloat16(), bias=bias.bfloat16(), r1=r1.bfloat16(), r2=r2.bfloat16(), upsample=upsample)


def conv_args(inp, arms):
    """keyword arguments of conv_ref64 / conv_model for one epilogue-arm selection (ARMS_NONE's keys) -- without x"""
    return dict(w=inp["w"], bias=inp["bias"] if arms["bias"] else None, r1=inp["r1"] if arms["r1"] else None, a1=A1,
                r2=inp["r2"] if arms["r2"] else None, a2=A2, slope=SLOPE, act=arms["act"], upsample=arms["upsample"])


def conv_gate(inp, arms):
    cin = inp["w"].shape[-1]
    ref, A = conv_ref64(inp["xbuf"][..., :cin], **conv_args(inp, arms))
    bound = U_BF16 * ref.abs() + (9 * cin + 4) * 2.0 ** -24 * A
    return dict(ref=ref, bound=bound)


def conv_check(got, g):
    """(number of elements beyond MARGIN * bound, worst err / bound) for got [B, H, W, Cout]"""
    got = got.detach().cpu()
    assert got.shape == g["ref"].shape, f"shape {tuple(got.shape)} vs {tuple(g['ref'].shape)}"
    assert torch.isfinite(got.float()).all(), "output not finite"
    n_bad = int(((got.double() - g["ref"]).abs() > MARGIN * g["bound"]).sum())
    return n_bad, _worst_ratio(got, g["ref"], g["bound"])


# ---- the whole network (BasicSR "new" key layout, float tensors holding bf16 values) -------------------------------------------------
def _net(sd, x, conv, num_block):
    """conv(x, name, **epilogue) -> [B, H, W, Cout]; x [B, H, W, 3]"""
    feat = conv(x, "conv_first")
    h = feat
    for i in range(num_block):
        x0 = h
        for j in (1, 2, 3):
            parts = [h]
            for k in (1, 2, 3, 4):
                parts.append(conv(torch.cat(parts, -1), f"body.{i}.rdb{j}.conv{k}", act=True))
            h = conv(torch.cat(parts, -1), f"body.{i}.rdb{j}.conv5", r1=h, a1=0.2, **(dict(r2=x0, a2=0.2) if j == 3 else {}))
    t = conv(h, "conv_body", r1=feat, a1=1.0)
    t = conv(t, "conv_up1", act=True, upsample=2)
    t = conv(t, "conv_up2", act=True, upsample=2)
    t = conv(t, "conv_hr", act=True)
    return conv(t, "conv_last")


def _num_block(sd):
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("body."))


def _wb(sd, name, dtype):
    return sd[name + ".weight"].permute(0, 2, 3, 1).to(dtype), sd[name + ".bias"].to(dtype)


def net_ref64(sd, x):
    """fp64 everywhere, no rounding between layers; sd: BasicSR keys, x [B, H, W, 3] -> [B, 4H, 4W, 3]"""
    def conv(t, name, **kw):
        w, b = _wb(sd, name, torch.float64)
        return _conv(t, w, b, kw.get("r1"), kw.get("a1", 1.0), kw.get("r2"), kw.get("a2", 1.0), SLOPE, kw.get("act", False),
                     kw.get("upsample", 1), torch.float64)
    return _net(sd, x.double(), conv, _num_block(sd))


def net_model(sd, x, order=0):
    """fp32 inside a launch, ONE bf16 rounding per launch: the network as the kernel's contract defines it"""
    def conv(t, name, **kw):
        w, b = _wb(sd, name, torch.float32)
        return _conv(t, w, b, kw.get("r1"), kw.get("a1", 1.0), kw.get("r2"), kw.get("a2", 1.0), SLOPE, kw.get("act", False),
                     kw.get("upsample", 1), torch.float32, order).bfloat16().float()
    return _net(sd, x.float(), conv, _num_block(sd))


def net_figures(got, ref):
    """(rel-L2, max abs error) of got against the fp64 reference"""
    return _rel_l2(got.detach().cpu(), ref), (got.detach().cpu().double() - ref).abs().max().item()
