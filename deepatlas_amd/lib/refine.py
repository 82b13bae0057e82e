"""Instance refinement of a displacement field: VoxelMorph's "instance-specific optimisation".  The field a registration net predicts for a
pair is a starting point; a few dozen Adam iterations on the similarity of this very pair, under the regulariser the net was trained with,
improve it without labels or retraining.

refine_field(fused=True) runs three launches per iteration (csrc/refine.hip): da_refine_moments (the five sums of NCC through the warp, the
warped image never written), da_bending_bwd (the regulariser's gradient into a scratch field) and da_refine_step (similarity gradient +
that field -> Adam on the field, in place).  fused=False is the same optimisation composed from the existing ops through autograd (WarpFn,
the loss modules of lib/loss.py, da_adam_step): the route of the other similarities and of the folding penalty, and the comparator of
tools/bench_refine.py.

Units.  The field is WarpFn's: N x 3 x D x H x W, channels (x, y, z) = (W, H, D) axis, normalised to [-1, 1].  `lr_vox` is Adam's step in
VOXELS: channel c steps by lr_vox * 2 / (extent_c - 1) (ops.refine_lr3), the same distance on every axis of a non-cubic volume, and by 0
along an axis of extent 1.  `grad_scale` multiplies the gradient before Adam sees it and defaults to the number of voxels V: the raw gradient
of a mean over V voxels is of the order 1 / V (1e-6 .. 1e-7 at the usual sizes), where Adam's eps = 1e-8 would no longer be negligible beside
sqrt(v) and the step would depend on the volume's size; scaled by V the gradient is of order 1 and eps is what it is in training.
"""
import torch

from .loss import BendingEnergyLoss, JacobianFoldingLoss
from .affine import make_sim, SIM_LOSSES
from .. import ops
from .._native import call, ptr, stream

FUSED_SIMS = ('ncc',)


def check_settings(iters=50, lr_vox=0.1, lambda_sim=1.0, lambda_reg=1.0, sim='ncc', fused=True, lambda_jac=0.0, **_):
    """The argument checks of refine_field that need no device (also run on config['refine'] and the command line)."""
    if isinstance(iters, bool) or int(iters) != iters or iters < 0:
        raise ValueError('iters must be an integer >= 0, got %r' % (iters,))
    for name, val in (('lr_vox', lr_vox), ('lambda_sim', lambda_sim), ('lambda_reg', lambda_reg), ('lambda_jac', lambda_jac)):
        if not 0.0 <= float(val) < float('inf'):
            raise ValueError('%s must be finite and >= 0, got %r' % (name, val))
    if sim not in SIM_LOSSES:
        raise ValueError("sim must be one of %s, got %r" % (', '.join(sorted(SIM_LOSSES)), sim))
    if fused and sim not in FUSED_SIMS:
        raise ValueError("the fused refinement supports sim = %s; %r runs with fused=False" % (' | '.join(repr(s) for s in FUSED_SIMS), sim))
    if fused and float(lambda_jac) > 0.0:
        raise ValueError('the folding penalty (lambda_jac > 0) runs with fused=False')


REFINE_KEYS = ('iters', 'lr_vox', 'lambda_sim', 'lambda_reg', 'sim', 'reg_settings', 'betas', 'eps', 'grad_scale', 'fused', 'graph', 'sim_settings',
               'lambda_jac', 'jac_settings')


def settings_from_config(cfg, refine):
    """The refine_field keywords of an experiment or a checkpoint's train_config.json: `refine` is None (off), an iteration count or a dict
    of refine_field keywords; what it leaves open comes from the config the net was trained with -- lambda_reg = config['lambda_reg'], sim =
    config['sim_loss'] with config['sim_settings'], and fused exactly when that similarity has a fused route.  Returns None or the complete,
    checked dict.  Needs no device."""
    if refine is None:
        return None
    if isinstance(refine, bool) or not isinstance(refine, (int, dict)):
        raise ValueError("config['refine'] must be None, an iteration count or a dict of refine_field keywords, got %r" % (refine,))
    given = dict(refine) if isinstance(refine, dict) else {'iters': refine}
    unknown = sorted(set(given) - set(REFINE_KEYS))
    if unknown:
        raise ValueError("config['refine'] has unknown keys %s (known: %s)" % (', '.join(unknown), ', '.join(REFINE_KEYS)))
    out = {'lambda_reg': float(cfg.get('lambda_reg', 1.0)), 'sim': cfg.get('sim_loss') or 'ncc'}
    out.update(given)
    if out['sim'] == (cfg.get('sim_loss') or 'ncc') and 'sim_settings' not in out and cfg.get('sim_settings'):
        out['sim_settings'] = dict(cfg['sim_settings'])
    out.setdefault('fused', out['sim'] in FUSED_SIMS and not float(out.get('lambda_jac') or 0.0) > 0.0)
    check_settings(**out)
    return out


def one_minus_ncc(moving, fixed, disp, per_sample=False):
    """1 - NCC(WarpFn(moving, disp), fixed) as a device tensor, the mean over the batch (0-d) or with per_sample one value per sample [N]: one
    pass, the warped image never written."""
    mv, fx, N, D, H, W = ops.refine_args(moving, fixed, disp)
    with torch.cuda.device(mv.device):
        stats = ops.refine_moments(mv, fx, ops.ndhwc(disp.detach()))
    return (1.0 - stats[:, 5]).float() if per_sample else (1.0 - stats[:, 5].mean()).float()


def _states(iters, lr3, betas, eps, grad_scale, lambda_sim, device):
    """iters x REFINE_STATE_FLOATS on the device, one host-to-device copy: row i holds the scalars of Adam step i + 1 and history slot i."""
    if iters == 0:
        return torch.empty((0, ops.REFINE_STATE_FLOATS), dtype=torch.float32, device=device)
    return torch.stack([ops.refine_host_state(lr3, betas, eps, i + 1, grad_scale, lambda_sim, i) for i in range(iters)]).to(device)


def _refine_fused(mv, fx, u, iters, lr3, lambda_sim, lambda_reg, bend, betas, eps, grad_scale, graph):
    N, D, H, W = (int(s) for s in u.shape[:4])
    dev = u.device
    m, v = torch.zeros_like(u), torch.zeros_like(u)
    hist = torch.zeros((iters,), dtype=torch.float32, device=dev)
    if iters == 0:
        return hist
    states = _states(iters, lr3, betas, eps, grad_scale, lambda_sim, dev)
    state = states[0].clone()
    stats = torch.empty((N, 8), dtype=torch.float64, device=dev)
    # a workspace of this loop's own: a captured launch keeps its pointer, and the shared one may be replaced by a later, larger request
    wsb = int(ops.nat.lib().da_refine_moments_ws_bytes(N, D, H, W))
    wbuf = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    ws = (ptr(wbuf), ops.ctypes.c_size_t(wsb))
    gx = torch.empty_like(u) if lambda_reg > 0.0 else None
    gl = torch.full((1,), float(lambda_reg), dtype=torch.float32, device=dev)
    sp, normalize, norm = ops.ctypes_float3(tuple(float(s) for s in bend.spacing)), 1 if bend.normalize else 0, 2 if bend.norm == 'L2' else 1

    def iteration(update=True, scratch=None):
        # the launch arguments do not depend on the iteration: its scalars are in `state`
        ops.refine_moments(mv, fx, u, stats, ws)
        if gx is not None:
            call('da_bending_bwd', ptr(u), ptr(gl), ptr(gx), N, D, H, W, sp, normalize, norm, stream())
        ops.refine_step(mv, fx, u, stats, state, g_extra=gx, m=m, v=v, hist=hist if update else None, grad_out=scratch, update=update)

    g = None
    if graph:
        iteration(update=False, scratch=torch.empty_like(u))      # every kernel has run once before the capture; nothing is modified
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            iteration()
    for i in range(iters):
        state.copy_(states[i])
        if g is not None:
            g.replay()
        else:
            iteration()
    return hist


def _refine_composed(moving, fixed, u0, iters, lr3, lambda_sim, lambda_reg, crit, bend, lambda_jac, jac, betas, eps, grad_scale):
    """The same optimisation through autograd.  da_adam_step has one learning rate per call, so the parameters, their gradient and the moments
    are kept channel-planar (3 x N x D x H x W, a channel contiguous) and each channel takes its own call with lr3[c]."""
    N, D, H, W = (int(s) for s in u0.shape[:4])
    dev = u0.device
    p = u0.permute(4, 0, 1, 2, 3).contiguous()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hist = torch.zeros((iters,), dtype=torch.float32, device=dev)
    n = p[0].numel()
    for i in range(iters):
        disp = p.permute(1, 0, 2, 3, 4).detach().contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
        with torch.enable_grad():
            l_sim = crit(ops.WarpFn.apply(moving, disp)[0], fixed)
            loss = lambda_sim * l_sim
            if lambda_reg > 0.0:
                loss = loss + lambda_reg * bend(disp)
            if jac is not None:
                loss = loss + lambda_jac * jac(disp)
        grad, = torch.autograd.grad(loss, disp)
        hist[i] = l_sim.detach()
        g = grad.permute(1, 0, 2, 3, 4).contiguous()
        for c in range(3):
            call('da_adam_step', ptr(p[c]), ptr(g[c]), ptr(m[c]), ptr(v[c]), n, float(lr3[c]), float(betas[0]), float(betas[1]), float(eps), i + 1,
                 float(grad_scale), stream())
    return p.permute(1, 0, 2, 3, 4), hist


def refine_field(moving, fixed, disp0, iters=50, lr_vox=0.1, lambda_sim=1.0, lambda_reg=1.0, sim='ncc', reg_settings=None, betas=(0.9, 0.999),
                 eps=1e-8, grad_scale=None, fused=True, graph=False, return_history=False, sim_settings=None, lambda_jac=0.0, jac_settings=None):
    """`iters` Adam iterations on  lambda_sim * sim(WarpFn(moving, disp), fixed) + lambda_reg * BendingEnergyLoss(**reg_settings)(disp)
    [+ lambda_jac * JacobianFoldingLoss(**jac_settings)(disp)]  starting from disp0; returns the refined field, N x 3 x D x H x W float32 in
    disp0's units.  disp0 is not modified.  moving, fixed: N x 1 x D x H x W float32 on the GPU, N <= 64.
    lr_vox, grad_scale: see the module text (voxels per step; default grad_scale = D H W).  reg_settings: the constructor arguments of
    BendingEnergyLoss (norm, spacing, normalize); None is what the experiments train with.
    fused=True (sim 'ncc' only, no folding penalty: a ValueError names what is supported) runs the three-launch iteration of csrc/refine.hip;
    fused=False composes the same optimisation from WarpFn, the loss modules and da_adam_step, for every similarity ('ncc' | 'lncc' | 'mi'
    with sim_settings) and the folding penalty, on volumes of >= 2 voxels per axis.  graph=True (fused only) captures one iteration as a HIP graph -- a linear chain on one
    stream -- and replays it; the result is bit-identical to the eager loop.  return_history: also the `iters` values of the similarity
    loss (1 - NCC for 'ncc') BEFORE each update, a device tensor; the loop never synchronises with the host."""
    check_settings(iters=iters, lr_vox=lr_vox, lambda_sim=lambda_sim, lambda_reg=lambda_reg, sim=sim, fused=fused, lambda_jac=lambda_jac)
    if graph and not fused:
        raise ValueError('graph=True replays the fused iteration; the composed route (fused=False) runs eagerly')
    mv, fx, N, D, H, W = ops.refine_args(moving, fixed, disp0)
    if not fused and min(D, H, W) < 2:
        raise ValueError('the composed route warps with WarpFn, which needs >= 2 voxels per axis; an extent of 1 runs with fused=True (got %s)' % ((D, H, W),))
    iters, lambda_sim, lambda_reg, lambda_jac = int(iters), float(lambda_sim), float(lambda_reg), float(lambda_jac)
    lr3 = ops.refine_lr3(lr_vox, (D, H, W))
    grad_scale = float(D * H * W) if grad_scale is None else float(grad_scale)
    bend = BendingEnergyLoss(**dict(reg_settings or {}))
    with torch.cuda.device(mv.device), torch.no_grad():
        u = ops.ndhwc(disp0.detach()).clone()
        if fused:
            hist = _refine_fused(mv, fx, u, iters, lr3, lambda_sim, lambda_reg, bend, betas, eps, grad_scale, graph)
            out = ops.ncdhw(u)
        else:
            crit = make_sim(sim, sim_settings, mv.device)
            jac = JacobianFoldingLoss(**dict(jac_settings or {})) if lambda_jac > 0.0 else None
            out, hist = _refine_composed(moving.detach(), fixed.detach(), u, iters, lr3, lambda_sim, lambda_reg, crit, bend, lambda_jac, jac, betas,
                                         eps, grad_scale)
    return (out, hist) if return_history else out
