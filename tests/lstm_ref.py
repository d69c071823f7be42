"""Plain torch, fp64, CPU restatement of ONE bidirectional LSTM layer's recurrence in the interface of remfx_amd/csrc/lstm.hip
(rfx_lstm_fwd / rfx_lstm_bwd): the dense parts (input projection, dX, dW) are not here, the caller has them as matmuls.

Layout as in the kernels: channel-major [C][P], P = T * Bn, position t * Bn + b; gate order i, f, g, o.
  forward : xp [2][4H][P], W_hh, W_hh_reverse [4H][H]  ->  out [2H][P], gates [2][4H][P] (post-activation), cstate [2][H][P]
  backward: gout [2H][P], gates, cstate, the weights    ->  dG [2][4H][P] (gradients of the gate pre-activations)

Operand modes of the recurrent product (everything else -- cell update, accumulation, activations -- is unrounded):
  exact   no rounding;
  bf16    RFX_PREC_BF16: W_hh rounded to bf16 (RNE, lstm_pack_kernel / lstm_pack_local_kernel), the moving operand (h_{t-1}; in the
          backward sweep the four gate-gradient slices) rounded to bf16 (RNE, rfx_cvt_pk_bf16), one product;
  bf16x3  any other prec: W = hi + lo (RNE, then RNE of the residual), the moving operand split as split_hi_lo does (hi = the top
          16 bits, lo = the residual + 0x8000, truncated), product = hi.hi + hi.lo + lo.hi.
The backward sweep consumes the gates / cstate it is GIVEN (the kernels' own saved state in the GPU tests).

`perturb` (the noise floor of tests/test_lstm_ref_cpu.py and tests/test_gpu_lstm_kernel.py): every step's h (backward: dh) is
multiplied by 1 + perturb * N(0, 1) -- a model of 1-ulp exp / rcp and of another fp32 summation order.
`mutate`: one of MUTATIONS, a deliberately wrong recurrence (the faults the tight bound of the GPU tests has to see)."""
import torch

from tests.ref_common import bf16_rne, bf16_trunc  # noqa: F401

MODES = ("exact", "bf16", "bf16x3")
# name -> modes it applies to, sweeps it applies to
MUTATIONS = {
    "operand_unrounded": (("bf16",), ("fwd", "bwd")),          # h (gate gradients) not rounded
    "operand_truncated": (("bf16",), ("fwd", "bwd")),          # ... rounded by truncation instead of RNE
    "w_lo_dropped": (("bf16x3",), ("fwd", "bwd")),             # lo fragment of W_hh lost
    "stale_block": (("bf16", "bf16x3"), ("fwd", "bwd")),       # one 16-unit block of the moving operand is one step old
    "last_kstep_omitted": (("bf16", "bf16x3"), ("fwd", "bwd")),  # last 16 of the contraction left out
    "f_g_swapped": (("bf16", "bf16x3"), ("fwd", "bwd")),       # f and g gates of one unit swapped
    "reverse_starts_late": (("bf16", "bf16x3"), ("fwd", "bwd")),  # reverse direction begins its recurrence at t = T - 2
    "cprev_from_buffer": (("bf16", "bf16x3"), ("bwd",)),       # c_{-1} read from the (clamped) buffer position instead of 0
}


def _f32_bits(x):
    return x.to(torch.float32).contiguous().view(torch.int32)


def _from_bits(u, like):
    return u.view(torch.float32).to(like.dtype)


def split_w(w):
    """lstm_pack_kernel: hi = RNE(w), lo = RNE(w - hi)"""
    w32 = w.to(torch.float32)
    hi = bf16_rne(w32)
    lo = bf16_rne(w32 - hi)                       # fp32 subtraction, exact
    return hi.to(w.dtype), lo.to(w.dtype)


def split_hi_lo(v):
    """split_hi_lo of lstm.hip: hi = top 16 bits, lo = (bits(v - hi) + 0x8000) >> 16"""
    v32 = v.to(torch.float32)
    hi = bf16_trunc(v32)
    r = v32 - hi                                  # fp32, exact
    lo = _from_bits((_f32_bits(r) + 0x8000) & -65536, r)
    return hi.to(v.dtype), lo.to(v.dtype)


class _Product:
    """moving operand v [K][Bn] -> A . v with the mode's operand rounding; A = W_hh (forward) or W_hh^T (backward)"""

    def __init__(self, A, mode, mutate):
        assert mode in MODES, mode
        self.mode, self.mutate = mode, mutate
        if mutate == "last_kstep_omitted":
            A = A.clone()
            A[:, -16:] = 0
        if mode == "exact":
            self.hi, self.lo = A, None
        elif mode == "bf16":
            self.hi, self.lo = bf16_rne(A), None
        else:
            self.hi, self.lo = split_w(A)
            if mutate == "w_lo_dropped":
                self.lo = torch.zeros_like(self.lo)

    def __call__(self, v):
        if self.mode == "exact":
            return self.hi @ v
        if self.mode == "bf16":
            if self.mutate == "operand_unrounded":
                return self.hi @ v
            return self.hi @ (bf16_trunc(v) if self.mutate == "operand_truncated" else bf16_rne(v))
        vh, vl = split_hi_lo(v)
        return self.hi @ (vh + vl) + self.lo @ vh


def _noise(v, perturb, gen):
    if not perturb:
        return v
    return v * (1 + perturb * torch.randn(v.shape, generator=gen, dtype=torch.float64).to(v.dtype))


def _forward_dir(xp, W, mode, perturb, gen, mutate, late, operand_only=False):
    """xp [4][H][T][Bn] in PROCESSING order -> h [H][T][Bn], gates [4][H][T][Bn], c [H][T][Bn]"""
    _, H, T, Bn = xp.shape
    prod = _Product(W, mode, mutate)
    z = xp.new_zeros(H, Bn)
    h, hprev, c = z, z, z
    hs, gs, cs = [], [], []
    for s in range(T):
        if late and s == 1:                       # the recurrence proper starts here, from a zero state
            h, hprev, c = z, z, z
        v = _noise(h, perturb, gen) if operand_only else h
        if mutate == "stale_block":
            v = v.clone()
            v[16:32] = hprev[16:32]
        pre = xp[:, :, s] + prod(v).view(4, H, Bn)
        if mutate == "f_g_swapped":
            pre = pre.clone()
            pre[1, 0], pre[2, 0] = pre[2, 0].clone(), pre[1, 0].clone()
        i, f, o = torch.sigmoid(pre[0]), torch.sigmoid(pre[1]), torch.sigmoid(pre[3])
        g = torch.tanh(pre[2])
        c = f * c + i * g
        hprev, h = h, o * torch.tanh(c)
        if not operand_only:
            h = _noise(h, perturb, gen)
        hs.append(h)
        gs.append(torch.stack([i, f, g, o]))
        cs.append(c)
    return torch.stack(hs, 1), torch.stack(gs, 2), torch.stack(cs, 1)


def _backward_dir(gout, gates, c, W, mode, perturb, gen, mutate, late, operand_only=False):
    """gout [H][T][Bn], gates [4][H][T][Bn], c [H][T][Bn] in the forward PROCESSING order -> dG [4][H][T][Bn]"""
    H, T, Bn = gout.shape
    prod = _Product(W.t().contiguous(), mode, mutate)
    if mutate == "f_g_swapped":
        gates = gates.clone()
        gates[1, 0], gates[2, 0] = gates[2, 0].clone(), gates[1, 0].clone()
    z = gout.new_zeros(H, Bn)
    rec, dcc = z, z
    d, dprev = gout.new_zeros(4 * H, Bn), gout.new_zeros(4 * H, Bn)
    out = [None] * T
    for s in range(T - 1, -1, -1):
        first = s == 0 or (late and s == 1)       # the step whose predecessor state is zero
        if late and s == 0:
            rec, dcc = z, z                       # nothing flows back into the detached first step
        dh = gout[:, s] + rec
        if not operand_only:
            dh = _noise(dh, perturb, gen)
        i, f, g, o = gates[0, :, s], gates[1, :, s], gates[2, :, s], gates[3, :, s]
        cprev = c[:, s - 1] if not first else z
        if mutate == "cprev_from_buffer" and s == 0:
            cprev = c[:, 0]                       # what the clamped prefetch address holds
        th = torch.tanh(c[:, s])
        dc = dh * o * (1 - th * th) + dcc
        do = dh * th * o * (1 - o)
        di = dc * g * i * (1 - i)
        df = dc * cprev * f * (1 - f)
        dg = dc * i * (1 - g * g)
        dcc = dc * f
        out[s] = torch.stack([di, df, dg, do])
        dprev, d = d, torch.cat([di, df, dg, do])
        if s > 0:
            v = _noise(d, perturb, gen) if operand_only else d
            if mutate == "stale_block":
                v = v.clone()
                v[16:32] = dprev[16:32]
            rec = prod(v)
    return torch.stack(out, 2)


def _proc(x, d):
    """time axis (second to last) into the processing order of direction d, and back (an involution)"""
    return x if d == 0 else x.flip(-2)


def forward(xp, w_hh, w_hh_r, T, Bn, mode="exact", perturb=0.0, seed=0, mutate=None, dtype=torch.float64, operand_only=False):
    H = w_hh.shape[1]
    assert xp.shape == (2, 4 * H, T * Bn) and mutate in (None,) + tuple(MUTATIONS)
    gen = torch.Generator().manual_seed(seed)
    outs, gates, cst = [], [], []
    for d, W in enumerate((w_hh, w_hh_r)):
        x = _proc(xp[d].to(dtype).view(4, H, T, Bn), d)
        h, g, c = _forward_dir(x, W.to(dtype), mode, perturb, gen, None if mutate == "reverse_starts_late" else mutate,
                               mutate == "reverse_starts_late" and d == 1, operand_only)
        outs.append(_proc(h, d).reshape(H, T * Bn))
        gates.append(_proc(g, d).reshape(4 * H, T * Bn))
        cst.append(_proc(c, d).reshape(H, T * Bn))
    return torch.cat(outs), torch.stack(gates), torch.stack(cst)


def backward(gout, gates, cstate, w_hh, w_hh_r, T, Bn, mode="exact", perturb=0.0, seed=0, mutate=None, dtype=torch.float64,
             operand_only=False):
    H = w_hh.shape[1]
    assert gout.shape == (2 * H, T * Bn) and gates.shape == (2, 4 * H, T * Bn) and cstate.shape == (2, H, T * Bn)
    assert mutate in (None,) + tuple(MUTATIONS)
    gen = torch.Generator().manual_seed(seed)
    dG = []
    for d, W in enumerate((w_hh, w_hh_r)):
        go = _proc(gout[d * H:(d + 1) * H].to(dtype).view(H, T, Bn), d)
        g = _proc(gates[d].to(dtype).view(4, H, T, Bn), d)
        c = _proc(cstate[d].to(dtype).view(H, T, Bn), d)
        r = _backward_dir(go, g, c, W.to(dtype), mode, perturb, gen, None if mutate == "reverse_starts_late" else mutate,
                          mutate == "reverse_starts_late" and d == 1, operand_only)
        dG.append(_proc(r, d).reshape(4 * H, T * Bn))
    return torch.stack(dG)


# ---- the comparison the tests share ---------------------------------------------------------------------------------------------
FLOOR_PERTURB = 1e-7
FLIP_PERTURB = 1e-4
MARGIN = 8.0
# Floor of a case = |reference(perturb = FLOOR_PERTURB) - reference|, one draw with a fixed seed, and the bound of the GPU tests is
# MARGIN x floor.  Two things have to be added for that bound to be one an fp32 implementation of the SAME arithmetic can meet (both
# shown by this reference alone, tests/test_lstm_ref_cpu.py::test_fp32_copy_of_the_reference_meets_the_bound):
#  * FP32_TERM.  What the perturbation does not reach has a floor of exactly zero (T = 1: gates and cstate never see an h; the first
#    step of every case), while the kernels store fp32 and evaluate exp / rcp to 1 ulp: 16 fp32 half-ulps (2^-24) of the tensor's
#    scale -- a pre-activation sums H + 1 terms, an activation is two 1-ulp operations, the cell update four more products.  It is
#    1e-3 of what bf16 operand rounding moves the outputs by, so it takes nothing from what the bound can see.
#  * bf16 flips.  In the bf16 mode the rounding of the operand swallows a 1e-7 perturbation entirely unless the value sits on a
#    rounding boundary: gates / cstate then move by a whole bf16 ulp of one h.  At the sizes of the GPU cases one draw holds 0 - 2
#    such flips, so the literal floor is 0 for most cases and one flip's size for the others (fp32 copy of the reference against it:
#    360 x at H = 192, T = 6, Bn = 65).  The flip part of the floor is therefore estimated from a draw in which flips are common --
#    FLIP_PERTURB on the operand only, nf operands round differently -- scaled to FLOOR_PERTURB: the flip count is proportional to the
#    perturbation and the L2 error to its square root, so L2 x sqrt(max(FLOOR_PERTURB / FLIP_PERTURB, 1 / nf)); never less than ONE
#    flip, which is what an implementation either has or has not.  A single flip moves max-abs by the same amount however rare it
#    is: the max-abs floor is that draw's, unscaled.
FP32_TERM = 16 * 2.0 ** -24


def errors(a, b):
    """(relative L2, max-abs over max-abs) of a against b"""
    a, b = a.double(), b.double()
    return (float((a - b).norm() / b.norm().clamp_min(1e-300)), float((a - b).abs().max() / b.abs().max().clamp_min(1e-300)))


def per_direction(name, t, H):
    """[(label, tensor)] one entry per direction: out is [2H][P], the others [2][C][P]"""
    if name == "out":
        return [("out.d0", t[:H]), ("out.d1", t[H:])]
    return [(f"{name}.d{d}", t[d]) for d in range(2)]


def differences(ref, other, H):
    """{label: (l2, max)} of the tensors in the dicts ref / other (same keys), per direction"""
    fl = {}
    for name in ref:
        for (label, r), (_, n) in zip(per_direction(name, ref[name], H), per_direction(name, other[name], H)):
            fl[label] = errors(n, r)
    return fl


def floors(run, mode, H, operand):
    """run(perturb, operand_only) -> {name: tensor}.  Returns (reference tensors, {label: (floor_l2, floor_max)}); `operand` names
    the tensor whose bf16 rounding is the recurrent product's moving operand (out; dG in the backward sweep)."""
    ref = run(0.0, False)
    fl = differences(ref, run(FLOOR_PERTURB, False), H)
    if mode == "bf16":
        noisy = run(FLIP_PERTURB, True)
        f2 = differences(ref, noisy, H)
        for d in range(2):
            a, b = per_direction(operand, ref[operand], H)[d][1], per_direction(operand, noisy[operand], H)[d][1]
            nf = int((bf16_rne(a) != bf16_rne(b)).sum())
            s = max(FLOOR_PERTURB / FLIP_PERTURB, 1.0 / max(nf, 1)) ** 0.5
            for label in fl:
                if label.endswith(f".d{d}"):
                    fl[label] = (max(fl[label][0], s * f2[label][0]), max(fl[label][1], f2[label][1]))
    return ref, fl


def bound(floor):
    return MARGIN * floor + FP32_TERM


def forward_case(xp, w0, w1, T, Bn, mode, mutate=None, dtype=torch.float64):
    def run(perturb, operand_only):
        o, g, c = forward(xp, w0, w1, T, Bn, mode, perturb=perturb, seed=1, mutate=mutate, dtype=dtype, operand_only=operand_only)
        return {"out": o, "gates": g, "cstate": c}
    return run


def backward_case(gout, gates, cstate, w0, w1, T, Bn, mode, mutate=None, dtype=torch.float64):
    def run(perturb, operand_only):
        return {"dG": backward(gout, gates, cstate, w0, w1, T, Bn, mode, perturb=perturb, seed=2, mutate=mutate, dtype=dtype,
                               operand_only=operand_only)}
    return run


def make_inputs(H, T, Bn, seed=0):
    """fp32 xp ~ N(0, 1), W_hh, W_hh_reverse ~ U(+-1/sqrt(H)) (torch's default), gout ~ N(0, 1)"""
    g = torch.Generator().manual_seed(1000003 * seed + 4099 * H + 131 * T + Bn)
    k = H ** -0.5
    w = [(torch.rand(4 * H, H, generator=g) * 2 - 1) * k for _ in range(2)]
    xp = torch.randn(2, 4 * H, T * Bn, generator=g)
    gout = torch.randn(2 * H, T * Bn, generator=g)
    return xp, w[0], w[1], gout


# ---- the parameter glue of one bidirectional layer (rfx_lstm_cat_params, rfx_lstm_grad_scatter) ----------------------------------------
# Written as the operation: a concatenation, a sum of two biases and six additions -- each fp32 result is ONE rounding of the fp64 value
# (a copy: none), so the GPU test judges every element with bound 0.
GLUE_CASES = ((1, 1), (3, 5), (64, 48), (192, 192))             # (H, Cin)
GLUE_GRID = 1024 * 256                                          # threads of the capped grid
GLUE_PARAMS = ("w_ih", "w_ih_r", "b_ih", "b_hh", "b_ih_r", "b_hh_r")
GLUE_MUTATIONS = ("bcat_second_half_from_bh0", "gbh1_not_updated", "assign_for_add")


def forms_glue(H, Cin):
    """what one call of either entry reaches (both size their grid by the 2 * 4 H Cin weight elements); None: refused"""
    if H <= 0 or Cin <= 0:
        return None
    n = 2 * 4 * H * Cin
    out = {"weights", "biases"}
    if n > GLUE_GRID:
        out.add("stride_loop")
    if n % 256:
        out.add("ragged_last_block")
    return out                                                  # the 8 H biases take one pass of the same grid at every H below 32768


def glue_data(H, Cin):
    """every buffer with its own seed and scale, so that two exchanged pointers or halves show: the six parameters, the projection
    GEMM's gradients dwcat [8H][Cin] / dbcat [8H], and what the six gradient buffers hold before the call (nowhere zero)"""
    def rnd(n, seed, scale, shift=0.0):
        return (torch.randn(n, generator=torch.Generator().manual_seed(seed + 131 * H + Cin), dtype=torch.float64) * scale + shift).float()
    nw, nb = 4 * H * Cin, 4 * H
    p = {"w_ih": rnd(nw, 1, 1.0), "w_ih_r": rnd(nw, 2, 10.0), "b_ih": rnd(nb, 3, 0.1), "b_hh": rnd(nb, 4, 3.0),
         "b_ih_r": rnd(nb, 5, 30.0), "b_hh_r": rnd(nb, 6, 0.01)}
    d = {"dwcat": rnd(2 * nw, 7, 0.5), "dbcat": rnd(2 * nb, 8, 2.0)}
    g0 = {k: rnd(p[k].numel(), 11 + i, 1.0 + i, shift=5.0 * (i + 1)) for i, k in enumerate(GLUE_PARAMS)}
    return p, d, g0


def cat_params(p, mutate=None):
    """fp64 {wcat [8H Cin], bcat [8H]}"""
    second = p["b_ih_r"].double() + (p["b_hh"] if mutate == "bcat_second_half_from_bh0" else p["b_hh_r"]).double()
    return {"wcat": torch.cat([p["w_ih"], p["w_ih_r"]]).double(), "bcat": torch.cat([p["b_ih"].double() + p["b_hh"].double(), second])}


def grad_scatter(g, d, mutate=None):
    """fp64 {the six gradients after ONE call}: g + the half of dwcat / dbcat that belongs to it, both biases of a direction the same"""
    nw, nb = g["w_ih"].numel(), g["b_ih"].numel()
    add = {"w_ih": d["dwcat"][:nw], "w_ih_r": d["dwcat"][nw:], "b_ih": d["dbcat"][:nb], "b_hh": d["dbcat"][:nb], "b_ih_r": d["dbcat"][nb:],
           "b_hh_r": d["dbcat"][nb:]}
    out = {}
    for k in GLUE_PARAMS:
        if mutate == "gbh1_not_updated" and k == "b_hh_r":
            out[k] = g[k].double()
        elif mutate == "assign_for_add":
            out[k] = add[k].double()
        else:
            out[k] = g[k].double() + add[k].double()
    return out
