"""Inputs and the float64 reference of the inverse-consistency tests (test_invcons_reference.py on the CPU, test_gpu_invcons.py on the GPU).
Nothing here calls the code under test.

Definition (conventions of warp.hip: disp N x 3 x D x H x W, channels (x, y, z) = the (W, H, D) axes, normalised units, s_c = (size_c - 1) / 2):
    p(x) = identity(x) + u_a(x)
    r(x) = u_a(x) + T[u_b](p(x))            T = F.grid_sample(., 'bilinear', 'zeros', align_corners=True)
    L(u_a, u_b) = mean over the N V voxels of sum_c (s_c r_c(x))^2          voxels^2
    L_sym = (L(u_a, u_b) + L(u_b, u_a)) / 2
Reference: that formula in torch on the CPU in float64 on the float32 inputs, with the float64 identity of warp_cases.identity; the gradients
of both inputs come from autograd.  Per sample it also yields the statistics the forward reports: sum |s r|^2, sum |s r| (Euclidean norm),
max |s r| and the number of voxels whose sample point leaves [0, size - 1] on some axis.

Fields: regeval_cases.smooth_field(shape, n, amp, seed) + to_normalised(NOISE_SHARE amp randn) (seeded generator), then warp_cases.off_lattice.
The symmetric loss samples at identity + u_b as well, so BOTH fields of a case are moved off the lattice.

Conditioning: component k of d u_a jumps where the voxel coordinate p_k crosses an integer, and the outside count jumps at 0 and size - 1,
which are integers too.  A case is admissible only if warp_cases.lattice_distance >= warp_cases.DELTA for both of its fields.  That is a
condition on the inputs, asserted by test_invcons_reference.py; a seed that fails it is replaced, the rule is not.

Tolerances: the yardstick is the SAME formula evaluated in float32 on the CPU (float32 identity, float32 grid_sample).  FP32_DISTANCE holds,
per (case, amplitude), its distances from the float64 result as measured when the cases were written -- one direction: the loss (relative),
sum |s r|^2 and sum |s r| (relative, the largest over the samples), max |s r| (relative), the residual (max norm of s (r - r64) over max |s r64|), d u_a and d u_b (max norm over the
gradient's largest magnitude); symmetric: loss, d u_a, d u_b.  The kernels get FACTOR = 4 x those distances (another association, FMA
contraction, sums in double, a scatter in arrival order), but never less than the floors, which stand for the float32 arithmetic itself where
a recorded distance happens to be smaller than it:
  LOSS_FLOOR = 5e-7 (loss, each sample's sum |s r|^2 and sum |s r|): a tap weight is a product of three rounded fractions, a component of T a sum of eight rounded
    products, r one more addition and s r one more product: about eight roundings of 2^-24 = 6e-8 on a voxel's term, of which a mean over few
    voxels (2 x 2 x 2) keeps most;
  POINT_FLOOR = 2e-6 (the residual, max |s r|, both gradients): a single voxel's value additionally carries the float32 sample coordinate, five
    roundings on a normalised coordinate of magnitude <= 2 (warp_cases.COORD_ERR = 3e-7 (S - 1) / 2 voxels), times the slope of the sampled
    field, which the added noise makes of the order of the field's own size per voxel; a component of d u_a is a sum of eight differences of
    such products, d u_b a sum of the weighted contributions of every voxel that lands in the cell.  About 32 roundings of 2^-24.
test_invcons_reference.py re-measures the distances and checks that they still fit the bounds."""
import functools

import torch
import torch.nn.functional as F

import regeval_cases as rc
import warp_cases as wc

LOSS_FLOOR, POINT_FLOOR, FACTOR = 5e-7, 2e-6, 4.0
AMPS = (0.3, 2.0, 8.0)           # standard deviation of the smooth part, voxels; at 8 most samples of the small shapes leave the volume
NOISE_SHARE = 0.15               # iid noise added to it, as a share of the amplitude (0.3 voxels at 2)

# name: (D x H x W, N, what it is there for)
CASES = {
    '2x2x2':    ((2, 2, 2), 1, 'every tap on a border'),
    '2x3x5':    ((2, 3, 5), 2, 'batch 2'),
    '5x2x3':    ((5, 2, 3), 1, 'the short axis in the middle'),
    '7x9x66':   ((7, 9, 66), 1, 'a row of 66 voxels crosses a wavefront'),
    '5x7x29':   ((5, 7, 29), 1, '1015 voxels, 4 workgroups (fewer than 8: the plain grid-stride loop on more than one workgroup), the last one partly filled'),
    '17x30x22': ((17, 30, 22), 3, 'ragged, batch 3: 11220 voxels, 44 workgroups rounded down to 40: the XCD-contiguous split, some workgroups take a second round'),
    '33x47x61': ((33, 47, 61), 2, 'ragged, batch 2: 370 workgroups rounded down to 368, the XCD-contiguous split with ragged eighths'),
    '80x96x80': ((80, 96, 80), 1, '614400 voxels on the 2048 x 256 launch of both kernels: their grid-stride loops run more than once'),
}
IDS = list(CASES)
CASE_SEED = {name: 0 for name in IDS}            # a seed that fails the conditioning rule is replaced here
COMBOS = [(name, amp) for name in IDS for amp in AMPS]
COMBO_IDS = ['%s-amp%g' % c for c in COMBOS]

ONE_WAY = ('loss', 'sum2', 'mean', 'max', 'resid', 'd_a', 'd_b')
SYMMETRIC = ('loss', 'd_a', 'd_b')
FLOOR = dict(loss=LOSS_FLOOR, sum2=LOSS_FLOOR, mean=LOSS_FLOOR, max=POINT_FLOOR, resid=POINT_FLOOR, d_a=POINT_FLOOR, d_b=POINT_FLOOR)

# float32-torch-vs-float64 distances, measured on the CPU when the cases were written: (case, amplitude) -> (one direction: ONE_WAY, symmetric: SYMMETRIC)
FP32_DISTANCE = {
    ('2x2x2', 0.3): ((1.58e-08, 3.78e-08, 6.30e-09, 5.59e-08, 5.12e-08, 1.03e-07, 1.45e-07), (5.34e-08, 1.10e-07, 8.87e-08)),
    ('2x2x2', 2.0): ((2.26e-08, 3.25e-08, 1.75e-08, 5.78e-09, 3.54e-08, 1.73e-07, 1.58e-07), (8.20e-09, 1.73e-07, 9.42e-09)),
    ('2x2x2', 8.0): ((3.12e-08, 2.61e-08, 1.25e-08, 5.78e-09, 0.00e+00, 0.00e+00, 0.00e+00), (1.21e-08, 0.00e+00, 0.00e+00)),
    ('2x3x5', 0.3): ((1.00e-07, 4.16e-08, 1.89e-08, 1.57e-08, 1.45e-07, 3.91e-07, 2.05e-07), (1.30e-08, 3.70e-07, 2.13e-07)),
    ('2x3x5', 2.0): ((2.90e-08, 5.68e-09, 4.59e-09, 1.35e-08, 7.76e-08, 3.45e-07, 1.19e-07), (2.50e-09, 3.49e-07, 2.88e-07)),
    ('2x3x5', 8.0): ((8.36e-09, 5.89e-09, 3.85e-09, 1.35e-08, 2.56e-09, 4.52e-08, 4.48e-08), (1.71e-08, 4.52e-08, 4.32e-08)),
    ('5x2x3', 0.3): ((2.89e-08, 5.99e-08, 2.31e-08, 3.77e-08, 8.12e-08, 7.03e-08, 1.09e-07), (3.94e-09, 7.52e-08, 1.52e-07)),
    ('5x2x3', 2.0): ((1.75e-08, 3.49e-09, 2.31e-09, 8.41e-09, 5.11e-08, 1.29e-07, 1.04e-07), (3.74e-09, 1.07e-07, 5.69e-08)),
    ('5x2x3', 8.0): ((2.47e-08, 8.55e-09, 4.89e-09, 8.41e-09, 0.00e+00, 7.89e-08, 0.00e+00), (3.00e-09, 7.89e-08, 7.58e-08)),
    ('7x9x66', 0.3): ((3.93e-09, 9.41e-09, 4.03e-09, 2.72e-08, 2.24e-06, 2.29e-06, 3.59e-06), (2.41e-08, 2.25e-06, 1.75e-06)),
    ('7x9x66', 2.0): ((2.62e-08, 1.84e-10, 1.04e-09, 1.64e-08, 1.69e-06, 5.52e-06, 1.68e-06), (5.03e-08, 4.61e-06, 3.00e-06)),
    ('7x9x66', 8.0): ((8.34e-08, 8.58e-10, 6.62e-10, 3.12e-09, 1.54e-06, 3.19e-06, 3.44e-06), (3.49e-08, 3.14e-06, 1.60e-06)),
    ('5x7x29', 0.3): ((3.96e-08, 9.51e-09, 1.63e-09, 2.14e-07, 7.26e-07, 1.12e-06, 2.97e-06), (4.80e-09, 1.05e-06, 1.51e-06)),
    ('5x7x29', 2.0): ((1.01e-08, 2.67e-08, 1.21e-08, 1.12e-08, 1.10e-06, 2.21e-06, 2.10e-06), (2.09e-08, 2.24e-06, 8.83e-07)),
    ('5x7x29', 8.0): ((4.60e-08, 4.49e-10, 1.07e-09, 3.74e-08, 3.98e-07, 1.84e-06, 1.19e-06), (3.03e-08, 1.84e-06, 1.49e-06)),
    ('17x30x22', 0.3): ((1.89e-09, 1.15e-08, 4.86e-09, 1.61e-07, 1.31e-06, 2.96e-06, 1.49e-06), (2.59e-08, 2.10e-06, 1.18e-06)),
    ('17x30x22', 2.0): ((9.38e-08, 1.88e-08, 9.13e-09, 5.62e-07, 1.59e-06, 2.28e-06, 1.13e-06), (4.79e-08, 2.46e-06, 1.80e-06)),
    ('17x30x22', 8.0): ((1.50e-07, 7.87e-09, 3.63e-09, 6.00e-08, 1.44e-06, 2.26e-06, 1.50e-06), (1.20e-08, 2.26e-06, 2.38e-06)),
    ('33x47x61', 0.3): ((8.70e-08, 6.67e-09, 1.67e-09, 6.41e-08, 3.46e-06, 5.56e-06, 4.93e-06), (5.88e-08, 4.28e-06, 3.32e-06)),
    ('33x47x61', 2.0): ((1.64e-08, 1.30e-09, 2.63e-10, 6.77e-08, 3.04e-06, 4.40e-06, 1.26e-06), (2.44e-08, 4.32e-06, 5.53e-06)),
    ('33x47x61', 8.0): ((8.07e-08, 7.39e-09, 3.16e-09, 9.27e-08, 3.58e-06, 4.91e-06, 1.75e-06), (4.60e-08, 4.92e-06, 3.57e-06)),
    ('80x96x80', 0.3): ((9.14e-08, 5.22e-10, 8.17e-10, 1.89e-07, 5.55e-06, 9.79e-06, 1.29e-05), (3.11e-08, 8.37e-06, 7.03e-06)),
    ('80x96x80', 2.0): ((9.25e-08, 7.74e-09, 4.61e-09, 3.12e-08, 5.98e-06, 8.83e-06, 3.64e-06), (2.77e-08, 8.83e-06, 9.47e-06)),
    ('80x96x80', 8.0): ((9.19e-08, 1.20e-09, 7.23e-10, 9.57e-09, 8.61e-06, 9.48e-06, 3.09e-06), (1.92e-08, 9.48e-06, 9.22e-06)),
}


def bounds(name, amp, symmetric):
    """{quantity: bound} of a combination: 4 x the recorded float32 distances, not below the floors."""
    one, sym = FP32_DISTANCE[(name, amp)]
    keys, vals = (SYMMETRIC, sym) if symmetric else (ONE_WAY, one)
    return {k: max(FACTOR * v, FLOOR[k]) for k, v in zip(keys, vals)}


def make_field(shape, n, amp, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    rough = NOISE_SHARE * amp * torch.randn((n, 3) + tuple(shape), generator=g, dtype=torch.float64)
    u = (rc.smooth_field(shape, n, amp, seed) + rc.to_normalised(rough).float()).contiguous()
    return wc.off_lattice(u, tuple(shape)).contiguous()


@functools.lru_cache(maxsize=None)
def fields(name, amp):
    """(u_a, u_b) of a case: float32 N x 3 x D x H x W in normalised units, both off the lattice (never modified by a test)."""
    shape, n, _ = CASES[name]
    seed = CASE_SEED[name]
    return make_field(shape, n, amp, seed), make_field(shape, n, amp, seed + 50)


def scales(vol, dtype):
    D, H, W = vol
    return torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0], dtype=dtype).view(1, 3, 1, 1, 1)


def residual(u_a, u_b):
    """r = u_a + T[u_b](identity + u_a) in the dtype of the inputs (differentiable), normalised units."""
    vol = tuple(u_a.shape[2:])
    p = u_a + wc.identity(vol, u_a.dtype)
    return u_a + F.grid_sample(u_b, p.permute(0, 2, 3, 4, 1), mode='bilinear', padding_mode='zeros', align_corners=True)


def loss_of(u_a, u_b):
    """L(u_a, u_b), the definition, in the dtype of the inputs."""
    sr = residual(u_a, u_b) * scales(tuple(u_a.shape[2:]), u_a.dtype)
    return (sr * sr).sum(1).mean()


def outside_count(u_a):
    """per sample: voxels whose float64 sample point leaves [0, size - 1] on some axis or is not finite"""
    vol = tuple(u_a.shape[2:])
    c = wc.voxel_coords(u_a, vol)
    hi = wc._per_axis(vol, lambda s: float(s - 1))
    out = (~torch.isfinite(c) | (c < 0) | (c > hi)).any(1)
    return out.reshape(out.shape[0], -1).sum(1).double()


def evaluate(u_a, u_b, dtype):
    """One direction in `dtype` on the CPU: dict of loss (float), stats (float64 N x 4: sum |s r|^2, sum |s r|, max |s r|, outside), resid (float64
    N x 3 x D x H x W, normalised units), d_a, d_b (float64, by autograd)."""
    a = u_a.detach().cpu().to(dtype).requires_grad_(True)
    b = u_b.detach().cpu().to(dtype).requires_grad_(True)
    vol = tuple(a.shape[2:])
    r = residual(a, b)
    sr = r * scales(vol, dtype)
    q = (sr * sr).sum(1)
    loss = q.mean()
    loss.backward()
    with torch.no_grad():
        qn = q.detach().double().reshape(q.shape[0], -1)
        e = qn.sqrt()
        stats = torch.stack([qn.sum(1), e.sum(1), e.max(1).values, outside_count(u_a)], 1)
    return dict(loss=float(loss.detach().double()), stats=stats, resid=r.detach().double(), d_a=a.grad.double(), d_b=b.grad.double())


def symmetric_of(ab, ba):
    """L_sym and its gradients from the two directions' evaluations: ab = evaluate(u_a, u_b), ba = evaluate(u_b, u_a)."""
    return dict(loss=0.5 * (ab['loss'] + ba['loss']), d_a=0.5 * (ab['d_a'] + ba['d_b']), d_b=0.5 * (ab['d_b'] + ba['d_a']))


@functools.lru_cache(maxsize=None)
def reference(name, amp):
    """(one direction, symmetric) of a case in float64: computed once, shared by the tests, never modified."""
    u_a, u_b = fields(name, amp)
    ab = evaluate(u_a, u_b, torch.float64)
    return ab, symmetric_of(ab, evaluate(u_b, u_a, torch.float64))


def rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def rel_max(got, want):
    """max |got - want| / max |want| (the quantity's own scale); where the reference is zero everywhere (no sample inside the volume: d u_b of
    the 8-voxel amplitude on the smallest shapes) the absolute distance, which then has to be 0."""
    scale = float(want.abs().max())
    return float((got.detach().cpu().double() - want).abs().max()) / (scale if scale > 0 else 1.0)


def resid_distance(got, want):
    """max norm of s (r - r64) over max |s r64|: the residual's distance in voxels (got, want in normalised units)."""
    s = scales(tuple(want.shape[2:]), torch.float64)
    return float(((got.detach().cpu().double() - want) * s).abs().max() / (want * s).abs().max())


def one_way_distances(got, want):
    """ONE_WAY distances of an evaluation (dict as evaluate returns) from the reference's; the outside counts must agree exactly."""
    assert torch.equal(got['stats'][:, 3].cpu().double(), want['stats'][:, 3]), (got['stats'][:, 3], want['stats'][:, 3])
    gs, ws = got['stats'].cpu().double(), want['stats']
    d = dict(loss=rel(got['loss'], want['loss']), sum2=float(((gs[:, 0] - ws[:, 0]).abs() / ws[:, 0]).max()), mean=float(((gs[:, 1] - ws[:, 1]).abs() / ws[:, 1]).max()),
             max=float(((gs[:, 2] - ws[:, 2]).abs() / ws[:, 2]).max()), resid=resid_distance(got['resid'], want['resid']))
    for k in ('d_a', 'd_b'):
        if got.get(k) is not None:
            d[k] = rel_max(got[k], want[k])
    return d


def symmetric_distances(got, want):
    d = dict(loss=rel(got['loss'], want['loss']))
    for k in ('d_a', 'd_b'):
        if got.get(k) is not None:
            d[k] = rel_max(got[k], want[k])
    return d


def measure_fp32(name, amp):
    """The float32 evaluation's distances from the float64 reference: (ONE_WAY tuple, SYMMETRIC tuple)."""
    u_a, u_b = fields(name, amp)
    ab64, sym64 = reference(name, amp)
    ab = evaluate(u_a, u_b, torch.float32)
    sym = symmetric_of(ab, evaluate(u_b, u_a, torch.float32))
    one, s = one_way_distances(ab, ab64), symmetric_distances(sym, sym64)
    return tuple(one[k] for k in ONE_WAY), tuple(s[k] for k in SYMMETRIC)


def check(distances, bound, what):
    """Every measured distance within its bound; returns the distances."""
    for k, v in distances.items():
        assert v <= bound[k], '%s: %s is %.3e from float64 (bound %.1e)' % (what, k, v, bound[k])
    return distances


# ---- pinned lattice cases ------------------------------------------------------------------------------------------------------------
LATTICE_VOL, LATTICE_N = (5, 7, 11), 2


def lattice_fields(kind):
    """'zero': u_a = u_b = 0 (every output exactly 0).  'ua0': u_a = 0, u_b random (2 voxels): every sample point is a lattice point."""
    z = torch.zeros((LATTICE_N, 3) + LATTICE_VOL)
    return (z, z.clone()) if kind == 'zero' else (z, make_field(LATTICE_VOL, LATTICE_N, 2.0, 7))


def ref_d_a(inp, dtype, disp):
    """d L / d u_a at the field `disp` (the signature warp_cases.lattice_sides calls)."""
    return evaluate(disp, inp['u_b'], dtype)['d_a']


def lattice_sides(u_a, u_b):
    """(left, right) float64 d u_a of a lattice case: component k taken at u_a moved by -+ warp_cases.LATTICE_STEP voxel along axis k."""
    return wc.lattice_sides(ref_d_a, dict(disp=u_a, u_b=u_b, vol=tuple(u_a.shape[2:])))


# ---- translation pair ----------------------------------------------------------------------------------------------------------------
TRANSLATION_VOL, TRANSLATION_N, TRANSLATION_SHIFT = (5, 7, 11), 2, 1.5
# inside the volume the residual is (w0 + w1 - 1) x 1.5 voxels, w0 + w1 = (ix - x0) + (x0 + 1 - ix) in float32 at |ix| <= 10: two roundings of
# 2^-24 x 16, 3e-6 voxels; 1e-5 allows for the float32 coordinate itself
TRANSLATION_TOL_VOX = 1e-5


def translation_fields():
    """u_a = +1.5 voxels along x, u_b = -1.5: inverse translations; the sample points of the last two columns (x = W - 2, W - 1) leave the volume."""
    shape = (TRANSLATION_N, 3) + TRANSLATION_VOL
    k = torch.tensor([TRANSLATION_SHIFT, 0.0, 0.0], dtype=torch.float64).view(1, 3, 1, 1, 1)
    u = (k * wc.axis_scale(TRANSLATION_VOL)).float().expand(shape).contiguous()
    return u, (-u).contiguous()


# ---- non-finite fields ---------------------------------------------------------------------------------------------------------------
NONFINITE_VALUES = (float('nan'), 1e12)


def nonfinite_fields(value):
    """The 2x3x5 case at 2 voxels with `value` in one component of one voxel of u_a."""
    u_a, u_b = fields('2x3x5', 2.0)
    u_a = u_a.clone()
    u_a[1, 1, 1, 2, 3] = value
    return u_a, u_b


# ---- descent -------------------------------------------------------------------------------------------------------------------------
# Two smooth fields of DESCENT_AMP voxels at DESCENT_VOL, parametrised in voxels, Adam on both with DESCENT_LR voxel per step, DESCENT_STEPS steps
# on L_sym alone.  On the float64 reference L_sym goes from DESCENT_MEASURED[0] to DESCENT_MEASURED[1] (test_invcons_reference.py asserts the
# ratio with a margin of 4 below DESCENT_RATIO); the device has to end below DESCENT_RATIO x its initial loss.
DESCENT_VOL, DESCENT_AMP, DESCENT_LR, DESCENT_STEPS, DESCENT_RATIO = (17, 30, 22), 2.0, 0.05, 100, 0.1
DESCENT_MEASURED = (21.33, 0.460)          # ratio 0.0216


def descent_start():
    """(u_a, u_b) in VOXELS, float32 1 x 3 x D x H x W."""
    inv = 1.0 / wc.axis_scale(DESCENT_VOL)
    return tuple((rc.smooth_field(DESCENT_VOL, 1, DESCENT_AMP, seed).double() * inv).float() for seed in (3, 4))


def descent(loss_fn, u_a, u_b, device='cpu'):
    """Adam on both fields (voxels); loss_fn takes the normalised fields.  Returns the losses before each step and after the last."""
    scale = wc.axis_scale(DESCENT_VOL).to(u_a.dtype).to(device)
    a = u_a.clone().to(device).requires_grad_(True)
    b = u_b.clone().to(device).requires_grad_(True)
    opt = torch.optim.Adam([a, b], lr=DESCENT_LR)
    losses = []
    for _ in range(DESCENT_STEPS):
        opt.zero_grad()
        loss = loss_fn(a * scale, b * scale)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        losses.append(loss_fn(a * scale, b * scale).detach())
    return [float(l) for l in losses]


def sym_loss(u_a, u_b):
    return 0.5 * (loss_of(u_a, u_b) + loss_of(u_b, u_a))
