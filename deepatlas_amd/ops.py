"""torch.autograd.Function wrappers around the C-ABI launchers of libdeepatlas_hip.so.

Tensor convention at this layer: the *logical* shape is the reference's N x C x D x H x W, the *physical*
layout is dense channels-last ("NDHWC", torch.channels_last_3d strides).  `ndhwc(x)` returns the
N x D x H x W x C view (copying only when a caller hands in a differently-strided tensor); ops allocate
their outputs as N x D x H x W x C and return the permuted N x C x D x H x W view.

Every op is a HIP kernel launch on the current torch stream; there is no eager fallback.
"""
import ctypes
import os

import torch
from torch.autograd import Function

from . import _native as nat
from ._native import call, call_supported, ptr, stream, workspace


# ------------------------------------------------------------------------------------------------
# layout helpers
# ------------------------------------------------------------------------------------------------
def ndhwc(x):
    """N x C x D x H x W (any strides) -> dense N x D x H x W x C tensor (a view when already channels-last)."""
    nat.require_cuda(x)
    if x.dtype != torch.float32 and x.dtype != torch.bfloat16:
        raise nat.NativeError('deepatlas_amd kernels take fp32 tensors (bf16 for the activations of the bf16 storage mode); got %s' % x.dtype)
    xp = x.permute(0, 2, 3, 4, 1)
    return xp if xp.is_contiguous() else xp.contiguous()


def ncdhw(t):
    """dense N x D x H x W x C -> logical N x C x D x H x W view."""
    return t.permute(0, 4, 1, 2, 3)


def _empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


# ------------------------------------------------------------------------------------------------
# bf16 activation storage (BASELINE configs[4]; include/deepatlas_hip.h, last section)
# ------------------------------------------------------------------------------------------------
# 'fp32': every tensor fp32 (the reference's arithmetic).  'bf16': the tensors BETWEEN the layers of a network -- convolution / transposed
# convolution outputs, BatchNorm + activation outputs, pooled / up-sampled tensors and all their gradients -- are stored as bf16; network
# inputs, logits, displacement fields, everything the losses see, parameters, their gradients, statistics and every accumulation stay fp32.
# Goes with set_matrix_precision('bf16').  A kernel without a bf16 twin for some shape is bridged by conversion passes (call_act).
ACT_STORAGE_MODES = ('fp32', 'bf16')
ACT_STORAGE = 'fp32'


def set_activation_storage(mode):
    """Process-wide storage type of the network-internal activations; returns the previous mode."""
    global ACT_STORAGE
    if mode not in ACT_STORAGE_MODES:
        raise ValueError("activation storage must be one of %r, got %r" % (ACT_STORAGE_MODES, mode))
    prev, ACT_STORAGE = ACT_STORAGE, mode
    global LAZY_BN_UPSAMPLER
    LAZY_BN_UPSAMPLER = mode == 'bf16'
    return prev


def _act_dtype(channels=None):
    """dtype of a network-internal activation with `channels` channels (thin outputs -- the 3-channel displacement field -- stay fp32)."""
    if ACT_STORAGE == 'bf16' and (channels is None or (channels >= 8 and channels % 4 == 0)):
        return torch.bfloat16
    return torch.float32


class A(object):
    """Marks an activation / gradient tensor among the arguments of call_act (out=True: the kernel writes it)."""
    __slots__ = ('t', 'out')

    def __init__(self, t, out=False):
        self.t, self.out = t, out


def O(t):
    return A(t, True)


# bf16 twins whose activation arguments are not all bf16: expected pattern over the non-None activation arguments, in signature order
_TWIN_PATTERN = {'da_conv1x1_fwd': (1, 0), 'da_conv1x1_fwd_pro': (1, 0), 'da_conv1x1_dgrad': (0, 1), 'da_conv1x1_wgrad': (1, 0),
                 'da_conv1x1_wgrad_pro': (1, 0)}
BF16_FORCE_BRIDGE = False       # tests: take the conversion route even where a bf16 twin exists (A/B of every twin at network level)
bridged_calls = {}       # name -> number of calls that went through conversion passes (diagnostics: tests / bench report it)


def call_act(name, *args, may_decline=False):
    """call() for entry points with activation arguments (wrapped in A / O).  All fp32: the plain entry.  Some bf16: the `_bf16` twin when it
    exists and takes this combination natively; otherwise the bf16 tensors are converted to fp32 scratch tensors around the plain entry
    (inputs before, outputs after -- the stored values are the same, only passes are added).  may_decline: like call_supported."""
    acts = [a for a in args if isinstance(a, A) and a.t is not None]
    plain = lambda: [(ptr(a.t) if isinstance(a, A) else a) for a in args]
    if not any(a.t.dtype == torch.bfloat16 for a in acts):
        if may_decline:
            return call_supported(name, *plain())
        call(name, *plain())
        return True
    twin = name + '_bf16'
    pattern = tuple(1 if a.t.dtype == torch.bfloat16 else 0 for a in acts)
    if twin in nat.SIGNATURES and not BF16_FORCE_BRIDGE:
        if name in nat.BF16_MASKED_TWINS:
            mask, k = 0, 0
            for a in args:
                if isinstance(a, A):
                    if a.t is not None and a.t.dtype == torch.bfloat16:
                        mask |= 1 << k
                    k += 1
            if call_supported(twin, *(plain() + [mask])):
                return True
        elif pattern == _TWIN_PATTERN.get(name, (1,) * len(acts)):
            if call_supported(twin, *plain()):
                return True
    # bridge
    st = stream()
    conv, outs, keep = [], [], []          # keep: the fp32 scratch tensors stay referenced until the entry has been queued
    for a in args:
        if isinstance(a, A) and a.t is not None and a.t.dtype == torch.bfloat16:
            t32 = torch.empty(a.t.shape, dtype=torch.float32, device=a.t.device)
            keep.append(t32)
            if a.out:
                outs.append((a.t, t32))
            else:
                call('da_cast_bf16_to_f32', ptr(a.t), ptr(t32), a.t.numel(), st)
            conv.append(ptr(t32))
        elif isinstance(a, A):
            conv.append(ptr(a.t))
        else:
            conv.append(a)
    bridged_calls[name] = bridged_calls.get(name, 0) + 1
    if may_decline:
        if not call_supported(name, *conv):
            return False
    else:
        call(name, *conv)
    for t, t32 in outs:
        call('da_cast_f32_to_bf16', ptr(t32), ptr(t), t.numel(), st)
    del keep
    return True


def _ws(nbytes, like):
    return workspace.get(nbytes, like.device)


def _labels(t):
    """Index target -> (tensor kept alive, label_bytes).  uint8 and int64 are consumed in place."""
    nat.require_cuda(t)
    if t.dtype == torch.uint8:
        return t.contiguous(), 1
    if t.dtype != torch.int64:
        t = t.long()
    return t.contiguous(), 8


# ------------------------------------------------------------------------------------------------
# weight gradients on a side stream
# ------------------------------------------------------------------------------------------------
# The 3x3x3 weight-gradient kernels are MFMA-bound and off the critical path of the backward pass: nothing downstream needs dW
# before the optimiser step.  With ASYNC_WGRAD they run on a second HIP stream and ACCUMULATE straight into `weight.grad` (FlatAdam's
# flat bucket), so the HBM-bound BatchNorm / activation / pooling backward kernels of the following layers overlap with them
# instead of queueing behind them.  The consumer of the gradients (FlatAdam.zero_grad / step, parallel.allreduce_gradients) joins
# the side stream first.  Off by default: plain autograd semantics (p.grad valid on the current stream right after backward()).
ASYNC_WGRAD = False
_side_stream = None
_side_keep = []          # tensors the side stream still reads: referenced until the join instead of Tensor.record_stream(), whose
                         # event-polled frees made the caching allocator fall back to hipMalloc on random steps (40 -> 64 ms)


MATRIX_MODES = ('fp32', 'bf16', 'fp32_split')
# What the training entry points (SegmentationExperiment / train_seg.py, JointExperiment, bench.py) switch to unless told otherwise.  The C
# library itself starts in 'fp32' (mode 0): the kernel-variant bit-identity tests are written against the fp32 matrix instructions.
DEFAULT_MATRIX_PRECISION = 'fp32_split'


def set_matrix_precision(mode):
    """Arithmetic of the 3x3x3 convolutions on the matrix cores (process-wide; returns the previous mode):
    'fp32'        fp32 operands on the fp32 matrix instructions (one fmaf per product, like the reference's CPU convolution);
    'fp32_split'  fp32 operands scaled by a per-tile power of two and split into two fp16 terms (22 significand bits), three partial products
                  per multiply on the fp16 matrix pipe with fp32 accumulation.  Per product NARROWER than fp32 (bound 2^-21 + 2^-22 = 7e-7 against
                  fp32's 6e-8; an element more than 2^15..2^18 below its staged tile's maximum keeps an absolute 2^-40 of that maximum);
                  over the K >= 216 sums of these layers the error against double is not larger than 'fp32's (tests/test_gpu_split.py,
                  incl. the structured-outlier cases; csrc/split_f16.h states the bounds).  3/16 of the matrix time;
    'bf16'        operands ROUNDED to bf16 (BASELINE config 5); everything else stays fp32."""
    if mode not in MATRIX_MODES:
        raise ValueError("matrix precision must be one of %r, got %r" % (MATRIX_MODES, mode))
    from ._native import lib
    global _matrix_mode
    prev = lib().da_set_matrix_mode(MATRIX_MODES.index(mode))
    _matrix_mode = mode
    return MATRIX_MODES[prev]


# what the library was last told (it starts in 'fp32' unless DA_MATRIX_MODE says otherwise); only the kept-pack logic below reads it
_matrix_mode = {'1': 'bf16', '2': 'fp32_split'}.get(os.environ.get('DA_MATRIX_MODE', '0'), 'fp32')


# Every kernel of the package reduces in a fixed order (per-block partials + a second launch) except ONE: the scatter of the trilinear
# warp's gradient with respect to its SOURCE (only the joint step's 32-channel probability warp needs it), which uses float atomics.
# DETERMINISTIC switches that one to an order-independent fixed-point accumulation, making whole training steps run-to-run bit-identical.
DETERMINISTIC = os.environ.get('DA_DETERMINISTIC') == '1'
CHECK_LABELS = os.environ.get('DA_CHECK_LABELS') == '1'      # validate index targets of the cross-entropy family like torch does (host sync per call)


_nbt_pending = {}          # id(tensor) -> [tensor, count]: an alias bumped twice is ONE entry (a multi-tensor add over duplicates could race)
_NBT_FLUSH_AT = 256        # blocks used on their own, with another optimiser, never reach a flush hook: bound the list


def bump_batches_tracked(bn):
    """`bn.num_batches_tracked += 1` (nn.BatchNorm3d in training mode), deferred: one 4-us launch per BatchNorm layer in the dependent chain
    of a forward pass (17 per UNet_light step) becomes ONE multi-tensor launch when the network's forward returns (a forward hook the
    network classes register), at the next FlatAdam.step(), before any state_dict() of a module that owns a bumped counter (a state_dict
    pre-hook registered here), or when 256 distinct counters are pending."""
    t = bn.num_batches_tracked
    e = _nbt_pending.get(id(t))
    if e is None:
        _nbt_pending[id(t)] = [t, 1]
        if not getattr(bn, '_da_nbt_hooked', False):
            bn._da_nbt_hooked = True
            bn.register_state_dict_pre_hook(_nbt_state_dict_pre_hook)
        if len(_nbt_pending) >= _NBT_FLUSH_AT:
            flush_batches_tracked()
    else:
        e[1] += 1


def _nbt_state_dict_pre_hook(module, prefix, keep_vars):      # (a module-level function: a lambda here made every trained BatchNorm module unpicklable)
    flush_batches_tracked()


def flush_batches_tracked(*_):
    if _nbt_pending:
        ones = [e[0] for e in _nbt_pending.values() if e[1] == 1]
        if ones:
            torch._foreach_add_(ones, 1)
        for t, n in _nbt_pending.values():
            if n != 1:
                t.add_(n)
        _nbt_pending.clear()


def init_into(param, init_fn):
    """Fill a parameter with `init_fn` (an nn.init.*_ function) in the element order of a CONTIGUOUS tensor of its shape.  Tagged convolution
    weights are strided views of FlatAdam's tap-major buckets once an optimiser exists; a random fill of the view itself would walk
    memory order and hand the same random stream to different elements than the reference's contiguous parameter gets
    (lib/network_factory/unets.py:61-67): same seed, different weights.  Drawing into a contiguous temporary and copying keeps
    seed-for-seed reproducibility against the reference and against NATIVE_TIO = False."""
    with torch.no_grad():
        if param.data.is_contiguous():
            init_fn(param.data)
        else:
            tmp = torch.empty(param.shape, dtype=param.dtype, device=param.device)
            init_fn(tmp)
            param.data.copy_(tmp)


def set_deterministic(flag=True):
    global DETERMINISTIC
    prev, DETERMINISTIC = DETERMINISTIC, bool(flag)
    return prev


def enable_async_wgrad(flag=True):
    global ASYNC_WGRAD
    ASYNC_WGRAD = bool(flag)


def side_stream():
    """The second HIP stream; every caller is about to queue work on it."""
    global _side_stream, _side_dirty
    if _side_stream is None:
        _side_stream = torch.cuda.Stream(priority=0)
    _side_dirty = True
    return _side_stream


_side_dirty = False      # work has been queued on the side stream since the last join


def join_side_stream():
    """Make the current stream wait for every weight gradient issued on the side stream.  Nothing outstanding -> no stream
    dependency at all (inside a HIP-graph capture a wait on work from before the capture would be illegal)."""
    global _side_dirty
    if _side_stream is not None and (_side_dirty or _side_keep):
        torch.cuda.current_stream().wait_stream(_side_stream)
    _side_keep.clear()
    _side_dirty = False


_last_side_flops = 0.0          # FLOPs of the weight gradient most recently queued on the side stream


def _serialize_matrix_kernels(flops, voxels):
    """Called right before a matrix-bound data-gradient kernel is queued on the main stream: for a LARGE full-resolution data
    gradient (>= 3e11 FLOPs on >= 4e6 voxels) behind a much shorter queued weight gradient (<= 0.4 of its FLOPs) the main stream first
    waits for the side stream.  The conv kernels are persistent with a static tile partition; such a data gradient that starts
    while the short weight gradient drains its last workgroups gets its own workgroups started unevenly and finishes late (the
    48 <- 16 data gradient of UNet_light: 3.3 ms alone, 4.9 ms when it starts 0.7 ms before the 16 -> 16 weight gradient ends).
    Whether that happens depends on microseconds of launch timing -- removing sixteen 2-us fill kernels per step moved the step from
    38.7 to 40.9 ms -- so the schedule is pinned instead of left to chance: 39.05 ms in either case.  The rule is deliberately
    narrow: on coarse, few-tile layers (all of the full UNet below full resolution) overlapping MFMA kernels fill each other's
    tails and waiting costs 10 % (268 vs 300 ms per step), and equally long kernels are left to overlap too."""
    if (ASYNC_WGRAD and _side_stream is not None and _side_dirty and flops >= _SERIALIZE_MIN_FLOPS and voxels >= _SERIALIZE_MIN_VOXELS
            and _last_side_flops <= _SERIALIZE_MAX_RATIO * flops):
        torch.cuda.current_stream().wait_stream(_side_stream)


_SERIALIZE_MIN_FLOPS = 3e11
_SERIALIZE_MAX_RATIO = 0.4
_SERIALIZE_MIN_VOXELS = 4e6


def _run_on_side(fn, keep_alive):
    """Run `fn()` on the side stream after everything queued so far on the current stream; `keep_alive` tensors stay referenced
    until the join."""
    side = side_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    _side_keep.extend(t for t in keep_alive if t is not None)


_flat_buckets = []       # weak references to every FlatAdam gradient bucket alive in this process


def register_flat_bucket(flat_g):
    """FlatAdam announces its gradient bucket: only gradients that live inside such a bucket are accumulated asynchronously (their
    consumer -- FlatAdam.zero_grad / step, parallel.allreduce_gradients -- joins the side stream; any other optimiser would not)."""
    import weakref
    _flat_buckets[:] = [r for r in _flat_buckets if r() is not None]
    _flat_buckets.append(weakref.ref(flat_g))


def _in_flat_bucket(g):
    a = g.data_ptr()
    for r in _flat_buckets:
        b = r()
        if b is not None and b.device == g.device and b.data_ptr() <= a and a + 4 * g.numel() <= b.data_ptr() + 4 * b.numel():
            return True
    return False


def _async_target(param):
    """The tensor to accumulate an asynchronous gradient into, or None for the synchronous autograd path (frozen parameters,
    gradients that are not views of a registered FlatAdam bucket, ASYNC_WGRAD off)."""
    if not ASYNC_WGRAD or param is None or not isinstance(param, torch.nn.Parameter) or not param.requires_grad:
        return None
    g = param.grad
    if g is None or not g.is_cuda or g.dtype != torch.float32:
        return None
    if not g.is_contiguous() and _tio_native(g, getattr(param, '_da_kind', None)) is None:      # (a tap-major native gradient view is dense too)
        return None
    if not _in_flat_bucket(g):
        return None
    return g


# ------------------------------------------------------------------------------------------------
# weight layouts, converted once per optimiser step
# ------------------------------------------------------------------------------------------------
# The kernels take weights tap-major ([k^3][Cin][Cout], "TIO"); the parameters keep the reference's state_dict layouts.  A weight only
# changes when an optimiser steps (or a state_dict is loaded), so its TIO copy is cached ON the parameter object and rebuilt when
#   * FlatAdam stepped (its HIP kernel writes through raw pointers, so torch's version counters do not move: bump_weights_epoch()),
#   * the parameter or a registered flat parameter bucket was written in place (torch's _version), or its storage moved.
# Inside a HIP-graph capture the cache is bypassed (the conversion kernel must be part of the graph).
_weights_epoch = 0
_flat_param_buckets = []          # weak references to every FlatAdam parameter bucket


_other_bumps = 0                  # bumps that are not one optimiser's step (parameters moved into a bucket, broadcast, graph replay): everything is stale
_bucket_epoch = {}                # storage pointer of a FlatAdam parameter bucket -> number of its optimiser's steps


def bump_weights_epoch(flat_p=None):
    """Weights changed behind torch's version counters.  flat_p: only the parameters of that FlatAdam bucket (its step); None: anything."""
    global _weights_epoch, _other_bumps
    _weights_epoch += 1
    if flat_p is None:
        _other_bumps += 1
    else:
        k = flat_p.untyped_storage().data_ptr()
        _bucket_epoch[k] = _bucket_epoch.get(k, 0) + 1


def register_flat_params(flat_p):
    import weakref
    _flat_param_buckets[:] = [r for r in _flat_param_buckets if r() is not None]
    _flat_param_buckets.append(weakref.ref(flat_p))


# ------------------------------------------------------------------------------------------------
# packed convolution operands, kept across calls (include/deepatlas_hip.h: da_conv3d_k3_prepack / _use_prepacked)
# ------------------------------------------------------------------------------------------------
# In the split matrix mode every stride-1 3x3x3 forward / data-gradient call used to launch a 10-us pack kernel (weights into fragment order + tile
# table) in front of its matrix kernel: 27 launches in the dependent chain of a seg step.  The packs only change when the weights do, so they are
# kept per (weights, direction, shape): filled in-chain the first time, and from then on re-filled for ALL layers of an optimiser right after its
# step -- on the side stream, beside the start of the next forward pass -- with one event per entry that the consuming call waits for.
# An entry is valid while its stamp (weights epoch, version counters: the one of weight_tio) matches and the weights' base tensor is alive; it holds
# a weak reference to that base only.  Not inside a HIP-graph capture.  PACK_CACHE = False (tests) switches it off.
PACK_CACHE = True
_pack_entries = {}


class _Pack(object):
    __slots__ = ('bufs', 'stamp', 'event', 'base', 'view', 'args', 'disabled', 'storage', 'pversion', 'used')


def _pack_stamp(e):
    # pversion: the version counter of the PARAMETER the weights belong to (a Parameter whose .data is a view of the flat bucket keeps its own
    # counter), as seen at the last use; FlatAdam's kernel moves neither counter, hence the epochs -- the one of the entry's OWN bucket, so that the
    # other network's optimiser step (joint training) leaves it valid
    b = e.base()
    return (_other_bumps, _bucket_epoch.get(e.storage, 0), e.pversion, b._version if b is not None else -1)


def _pack_fill(e, w_tio, st):
    C1, C2, Cout, dgrad, N, D, H, W = e.args
    used = ctypes.c_int(0)
    b1 = e.bufs[1]
    call('da_conv3d_k3_prepack', ptr(w_tio), C1, C2, Cout, dgrad, N, D, H, W, ptr(e.bufs[0]), e.bufs[0].numel(),
         ptr(b1), b1.numel() if b1 is not None else 0, ctypes.byref(used), st)
    return used.value


def use_pack(w_tio, dgrad, C1, C2, Cout, N, D, H, W, stride=1, up2=False):
    """Right before a da_conv3d_k3_{fwd,fwd_bnstats,fwd_pro,dgrad} or da_upconv3d_k3_{fwd,dgrad} call: hand it the kept packed operand of these weights
    (filling it now if it is new or stale).  Only stride-1 layers keep packs (the split matrix kernels); no-op for stride 2 and the folded up-sampling, outside
    the split matrix mode, for weights that are not views of a live base tensor, and inside graph capture."""
    if stride != 1 or up2 or not PACK_CACHE or _matrix_mode != 'fp32_split' or w_tio.dtype != torch.float32 or torch.cuda.is_current_stream_capturing():
        return
    key = (w_tio.data_ptr(), dgrad, C1, C2, Cout, N, D, H, W)
    e = _pack_entries.get(key)
    sp = w_tio.untyped_storage().data_ptr()
    if e is not None and (e.base() is None or e.storage != sp):
        e = None                                        # (the address was reused by other weights)
    if e is None:
        # only weights that live in a registered FlatAdam parameter bucket (tap-major views of it, weight_tio): the bucket is the live base object
        base = next((r for r in _flat_param_buckets if r() is not None and r().untyped_storage().data_ptr() == sp), None)
        if base is None:
            return
        nbytes = nat.lib().da_conv3d_k3_pack_bytes(N, D, H, W, C1 + C2, Cout)
        e = _Pack()
        e.args, e.event, e.stamp, e.disabled, e.used = (C1, C2, Cout, dgrad, N, D, H, W), None, None, nbytes == 0, True
        e.base = base
        e.storage = sp
        e.view = (tuple(w_tio.shape), tuple(w_tio.stride()), w_tio.storage_offset())
        e.bufs = [None, None]
        if not e.disabled:
            e.bufs[0] = torch.empty((nbytes,), dtype=torch.uint8, device=w_tio.device)
            if dgrad and C2 > 0:
                e.bufs[1] = torch.empty((nbytes,), dtype=torch.uint8, device=w_tio.device)
        _pack_entries[key] = e
    if e.disabled:
        return
    e.pversion = w_tio._version
    e.used = True
    stamp = _pack_stamp(e)
    if e.stamp != stamp:
        if e.event is not None:                         # a side-stream re-fill of these buffers may still be in flight (weights changed again right after the step)
            torch.cuda.current_stream().wait_event(e.event)
        if _pack_fill(e, w_tio, stream()) == 0:
            e.disabled = True
            e.bufs = [None, None]
            return
        e.stamp, e.event = stamp, None
    elif e.event is not None:
        torch.cuda.current_stream().wait_event(e.event)
    b1 = e.bufs[1]
    nat.lib().da_conv3d_k3_use_prepacked(ptr(w_tio), ptr(e.bufs[0]), e.bufs[0].numel(), ptr(b1), b1.numel() if b1 is not None else 0)


def repack_after_step(flat_p):
    """FlatAdam.step() calls this behind its update kernel: every kept pack of weights that live in `flat_p` is re-filled on the side stream."""
    if not PACK_CACHE or not _pack_entries or _matrix_mode != 'fp32_split' or torch.cuda.is_current_stream_capturing():
        return
    sp = flat_p.untyped_storage().data_ptr()
    # only the packs a call asked for since the previous step of this bucket are re-filled (a validation size, random crops or sliding windows would
    # otherwise grow the per-step work with every shape ever seen); the others go stale (re-filled in their next call) and, past _PACK_KEEP shapes
    # idle for a step, are dropped
    all_mine = [(k, e) for k, e in _pack_entries.items() if not e.disabled and e.storage == sp and e.base() is not None]
    mine, idle = [], []
    for k, e in all_mine:
        if e.used:
            mine.append(e)
            e.used = False
        else:
            idle.append(k)
            e.stamp = None                              # stale: its next call re-fills it in the call's own chain
    dead = [k for k, e in _pack_entries.items() if e.base() is None] + (idle[:len(idle) - _PACK_KEEP] if len(idle) > _PACK_KEEP else [])
    for k in dead:
        _pack_entries.pop(k, None)
    if not mine:
        return
    n = len(mine)
    views = [torch.as_strided(e.base(), e.view[0], e.view[1], e.view[2]) for e in mine]
    PA, IA, SA = ctypes.c_void_p * n, ctypes.c_int * n, ctypes.c_size_t * n
    cols = list(zip(*[e.args for e in mine]))                   # C1, C2, Cout, dgrad, N, D, H, W
    used = IA()
    side = side_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call('da_conv3d_k3_prepack_many', n, PA(*[v.data_ptr() for v in views]), IA(*cols[0]), IA(*cols[1]), IA(*cols[2]), IA(*cols[3]),
             IA(*cols[4]), IA(*cols[5]), IA(*cols[6]), IA(*cols[7]),
             PA(*[e.bufs[0].data_ptr() for e in mine]), SA(*[e.bufs[0].numel() for e in mine]),
             PA(*[(e.bufs[1].data_ptr() if e.bufs[1] is not None else None) for e in mine]), SA(*[(e.bufs[1].numel() if e.bufs[1] is not None else 0) for e in mine]),
             used, stream())
        ev = torch.cuda.Event()
        ev.record(side)
    for e, v, u in zip(mine, views, used):
        if u == 0:
            e.disabled = True
            continue
        e.stamp, e.event = _pack_stamp(e), ev


_PACK_KEEP = 64          # kept packs idle for a whole optimiser step beyond this many are dropped (oldest first: dicts keep insertion order)


def clear_pack_cache():
    _pack_entries.clear()


_TIO_ENTRY = {'oik': 'da_w_oik_to_tio', 'iok': 'da_w_iok_to_tio', 'iok_flip': 'da_w_iok_flip_to_tio'}
_TIO_BACK = {'oik': 'da_w_tio_to_oik', 'iok': 'da_w_tio_to_iok', 'iok_flip': 'da_w_tio_to_iok_flip'}

# TAP-MAJOR NATIVE STORAGE.  FlatAdam lays the convolution weights (and their gradients / moments) out in its flat buckets tap-major --
# the kernels' [k^3][Cin][Cout] -- and hands the modules STRIDED VIEWS of the reference's shapes ([Cout][Cin][k,k,k] / [Cin][Cout][k,k,k]):
# state_dict keys, shapes and values are the reference's, Adam is elementwise (layout-agnostic), and the per-step layout conversions
# (one launch per weight each way) do not exist.  A parameter's kind comes from tag_conv_layouts(); a parameter without an optimiser
# (or with another one) stays contiguous in the reference layout and takes the conversion kernels + cache below.
NATIVE_TIO = True         # (tests: False keeps every conv weight contiguous in the reference layout)


def tag_conv_layouts(module):
    """Mark the conv weights of `module` with the layout kind the kernels read them in ('oik': nn.Conv3d, 'iok': nn.ConvTranspose3d with
    kernel 2; the k3 transposed convs of the full UNet are read tap-FLIPPED, which no view expresses: untagged).  Called by the networks'
    constructors; FlatAdam reads the tag."""
    for m in module.modules():
        w = getattr(m, 'weight', None)
        if isinstance(m, torch.nn.ConvTranspose3d):
            if w is not None and tuple(w.shape[2:]) == (2, 2, 2):
                w._da_kind = 'iok'
        elif isinstance(m, torch.nn.Conv3d) and w is not None:
            w._da_kind = 'oik'


def param_view(buf, off, p):
    """View of buf[off : off + p.numel()] with p's logical shape: tap-major storage for tagged conv weights, plain otherwise."""
    k = p.numel()
    flat = buf[off:off + k]
    kind = getattr(p, '_da_kind', None) if NATIVE_TIO else None
    if kind is not None and p.dim() == 5:
        s0, s1, a, b, c = (int(v) for v in p.shape)
        if kind == 'oik':
            return flat.view(a, b, c, s1, s0).permute(4, 3, 0, 1, 2)
        if kind == 'iok':
            return flat.view(a, b, c, s0, s1).permute(3, 4, 0, 1, 2)
    return flat.view(p.shape)


def _tio_native(t, kind):
    """[K3][Cin][Cout] VIEW of a parameter-layout tensor whose storage already is tap-major, else None."""
    if t is None or t.dim() != 5 or kind not in ('oik', 'iok'):
        return None
    v = t.permute(2, 3, 4, 1, 0) if kind == 'oik' else t.permute(2, 3, 4, 0, 1)
    if not v.is_contiguous():
        return None
    return v.reshape(v.shape[0] * v.shape[1] * v.shape[2], v.shape[3], v.shape[4])


def _from_tio_view(dw_tio, kind, shape):
    """Parameter-layout strided VIEW of a [K3][Cin][Cout] tensor (no kernel)."""
    s0, s1, a, b, c = (int(v) for v in shape)
    if kind == 'oik':
        return dw_tio.view(a, b, c, s1, s0).permute(4, 3, 0, 1, 2)
    return dw_tio.view(a, b, c, s0, s1).permute(3, 4, 0, 1, 2)


class WgradTarget(object):
    """Where an ASYNCHRONOUS weight-gradient kernel of a parameter writes.  `gw` is the parameter's gradient tensor in the flat bucket (None:
    take the synchronous autograd path).  out() -- called INSIDE the stream context the kernel runs in, so that a scratch tensor belongs to
    that stream's allocator pool -- returns the [K3][Cin][Cout] tensor to hand to the kernel; finish() folds it into the bucket:
      * tap-major native bucket, not written since FlatAdam.zero_grad(): the bucket slice itself (writing over zeros == accumulating),
      * native, already written this step: scratch, then one add into the slice,
      * reference-layout gradient: scratch, then the converting accumulate kernel."""
    __slots__ = ('gw', 'kind', 'like', 'direct', 'view', 'tmp')

    def __init__(self, param, kind, w_tio):
        self.gw = _async_target(param)
        self.kind, self.like, self.direct, self.view, self.tmp = kind, w_tio, False, None, None
        if self.gw is not None:
            self.view = _tio_native(self.gw, kind)
            if self.view is not None and getattr(param, '_da_gz', False):
                param._da_gz = False
                self.direct = True

    def out(self):
        if self.direct:
            return self.view
        self.tmp = torch.empty_like(self.like)
        return self.tmp

    def finish(self):
        if self.direct:
            return
        if self.view is not None:
            self.view.add_(self.tmp)
        else:
            grad_from_tio(self.tmp, self.kind, self.gw.shape, acc=self.gw)
        self.tmp = None


_NO_WGRAD_TARGET = type('NoTarget', (), {'gw': None})()


def grad_for_autograd(dw_tio, kind, param):
    """The gradient tensor handed to autograd for `param` from its [K3][Cin][Cout] gradient: a strided view when the parameter lives
    tap-major (no kernel), else the layout conversion."""
    if isinstance(param, torch.nn.Parameter):
        param._da_gz = False                        # autograd is about to accumulate into .grad
    if kind in ('oik', 'iok') and _tio_native(param.detach(), kind) is not None:
        return _from_tio_view(dw_tio, kind, param.shape)
    return grad_from_tio(dw_tio, kind, param.shape)


def weight_tio(weight, kind):
    """[K3][Cin][Cout] copy of a conv weight.  kind 'oik': nn.Conv3d [Cout][Cin][k^3]; 'iok': nn.ConvTranspose3d [Cin][Cout][k^3];
    'iok_flip': a k3/s1/p1 transposed conv used as a convolution (taps flipped)."""
    a_, b_ = int(weight.shape[0]), int(weight.shape[1])
    K3 = int(weight.shape[2] * weight.shape[3] * weight.shape[4])
    Cin, Cout = (b_, a_) if kind == 'oik' else (a_, b_)
    nv = _tio_native(weight.detach(), kind)
    if nv is not None:                         # tap-major native storage (FlatAdam): the kernels read the parameter's own memory
        return nv
    capturing = torch.cuda.is_current_stream_capturing()
    stamp = None
    if not capturing:
        stamp = (_weights_epoch, weight._version, weight.data_ptr(), kind,
                 tuple(r()._version for r in _flat_param_buckets if r() is not None))
        ent = getattr(weight, '_da_tio', None)
        if ent is not None and ent[0] == stamp:
            return ent[1]
    w_tio = torch.empty((K3, Cin, Cout), dtype=torch.float32, device=weight.device)
    call(_TIO_ENTRY[kind], ptr(weight.detach().contiguous()), ptr(w_tio), a_, b_, K3, stream())
    if stamp is not None:
        try:
            weight._da_tio = (stamp, w_tio)
        except AttributeError:
            pass
    return w_tio


def grad_from_tio(dw_tio, kind, shape, acc=None):
    """The gradient in the parameter's own layout from a [K3][Cin][Cout] gradient: a new tensor, or (acc given) accumulated into
    `acc` by the same kernel."""
    a_, b_ = int(shape[0]), int(shape[1])
    K3 = int(dw_tio.shape[0])
    if acc is not None:
        call(_TIO_BACK[kind] + '_acc', ptr(dw_tio), ptr(acc), a_, b_, K3, stream())
        return None
    dw = torch.empty(tuple(shape), dtype=torch.float32, device=dw_tio.device)
    call(_TIO_BACK[kind], ptr(dw_tio), ptr(dw), a_, b_, K3, stream())
    return dw


# ------------------------------------------------------------------------------------------------
# deferred BatchNorm + activation
# ------------------------------------------------------------------------------------------------
# In Conv -> BatchNorm -> LeakyReLU -> Conv chains (unets.py:24-39, 259-278) the activated tensor only exists to be read by the next
# 3x3x3 convolution.  With LAZY_BN the producer returns its RAW output together with the BatchNorm scale / shift, and the consumer's
# kernels apply `act(x * scale + shift)` while staging their input tile (da_conv3d_k3_fwd_pro / da_conv3d_k3_wgrad_pro): the apply
# pass and the activated tensor disappear, the arithmetic (and therefore every result) stays bit-identical
# (tests/test_gpu_nets.py::test_lazy_batchnorm_matches_materialised_activations).
# Measured at 160x192x160, batch 2.  In the HBM-bound head kernels the prologue is free; in the MFMA-bound 3x3x3
# kernels its 4 VALU operations per staged element are not: 16 -> 16 forward 1.17 -> 1.20 ms, weight gradient 1.22 -> 1.29 ms; 48 -> 16
# forward 3.26 -> 3.40 ms, weight gradient 3.69 -> 3.93 ms.  Conv -> conv and conv -> head links (LAZY_BN; tests turn it off):
# 39.15 -> 38.6 ms/step, and the activated tensors of those links are never allocated.  The up-sampler -> concat-conv link
# (LAZY_BN_UPSAMPLER; set_activation_storage turns it on with bf16 storage only) saves another 0.2 ms/step but moves the bench's
# roofline call onto the prologue variant of the 48 -> 16 forward (0.757 instead of 0.778 of the fp32 matrix peak for the same algorithmic FLOPs).
LAZY_BN = True
LAZY_BN_UPSAMPLER = False       # (bf16 storage: the prologue is cheaper there -- seg step 13.04 -> 12.61 ms; fp32: 27.70 -> 27.70 - 27.78)


class LazyAct(object):
    """A tensor whose per-channel affine + activation has not been applied yet.  `raw` carries the autograd history; the gradient
    that flows back into it is the gradient with respect to the ACTIVATED tensor (the producer's backward expects exactly that)."""
    __slots__ = ('raw', 'scale', 'shift', 'slope')

    def __init__(self, raw, scale, shift, slope):
        self.raw, self.scale, self.shift, self.slope = raw, scale, shift, float(slope)

    @property
    def shape(self):
        return self.raw.shape

    def materialize(self):
        return ApplyAffineActFn.apply(self.raw, self.scale, self.shift, self.slope)


def materialize(x):
    return x.materialize() if isinstance(x, LazyAct) else x


class ApplyAffineActFn(Function):
    """act(raw * scale + shift) as its own pass (da_bn_act_fwd) for consumers without an input prologue.  The incoming gradient is
    already the gradient with respect to the activated tensor, which is what `raw`'s producer expects: passed through unchanged."""

    @staticmethod
    def forward(ctx, raw, scale, shift, slope):
        a = ndhwc(raw)
        C = a.shape[-1]
        out = torch.empty_like(a)
        call_act('da_bn_act_fwd', A(a), ptr(scale), ptr(shift), float(slope), O(out), a.numel() // C, C, stream())
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        return gout, None, None, None


def _pro_args(pro):
    """(scale_ptr, shift_ptr, slope) of an optional prologue for the C entry points."""
    if pro is None:
        return None, None, -1.0
    return ptr(pro[0]), ptr(pro[1]), float(pro[2])


def _apply_pro(a, pro, st):
    """Materialise act(a * scale + shift) (fallback when a shape is not taken by the prologue kernels)."""
    if pro is None:
        return a
    C = a.shape[-1]
    out = torch.empty_like(a)
    call_act('da_bn_act_fwd', A(a), ptr(pro[0]), ptr(pro[1]), float(pro[2]), O(out), a.numel() // C, C, st)
    return out


# ------------------------------------------------------------------------------------------------
# convolutions
# ------------------------------------------------------------------------------------------------
class Conv3dK3Fn(Function):
    """nn.Conv3d(k=3, p=1, stride 1|2) on concat(x1, x2) (+ optional fused ReLU/LeakyReLU).
    Reference call sites: unets.py:30,36; modules.py:48,56-58; voxel_morph.py:57,82."""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, stride, act_slope, *extra):
        # extra[0] (optional): `weight` is a ConvTranspose3d(k=3, s=1, p=1) weight [Cin][Cout][3,3,3] (unets.py:88-96): the same
        # operation as this convolution with flipped taps, so only the weight re-layout kernels differ
        # extra[1] (optional): fork -- the output is returned TWICE (two aliases) for a tensor with two consumers (skip connection):
        # the two gradients then arrive separately and are summed inside the activation-backward pass instead of by autograd
        transposed = bool(extra[0]) if extra else False
        fork = bool(extra[1]) if len(extra) > 1 else False
        # extra[2] (optional): up2 -- x1 / x2 are the COARSE tensors of `conv(F.interpolate(x, scale 2, nearest))` (voxel_morph.py:72-80): the
        # up-sampling is folded into the convolution (conv3d_up2.hip), the up-sampled tensor and its gradient never exist
        up2 = bool(extra[2]) if len(extra) > 2 else False
        ctx.n_extra, ctx.transposed, ctx.fork, ctx.up2 = len(extra), transposed, fork, up2
        a1 = ndhwc(x1)
        a2 = ndhwc(x2) if x2 is not None else None
        N, D, H, W, C1 = a1.shape
        C2 = a2.shape[-1] if a2 is not None else 0
        Cout, Cin = (weight.shape[1], weight.shape[0]) if transposed else (weight.shape[0], weight.shape[1])
        if Cin != C1 + C2 or tuple(weight.shape[2:]) != (3, 3, 3):
            raise ValueError('weight %s does not match input channels %d+%d' % (tuple(weight.shape), C1, C2))
        if transposed and stride != 1:
            raise NotImplementedError('transposed 3x3x3 conv: stride 1 only')
        if up2 and (transposed or stride != 1 or not upconv_supported(C1, C2, Cout)):
            raise NotImplementedError('folded up-sampling: plain stride-1 convolution, channel counts of ops.upconv_supported, split matrix mode')
        st = stream()
        w_tio = weight_tio(weight, 'iok_flip' if transposed else 'oik')
        b = bias.detach().contiguous() if bias is not None else None
        if up2:
            out = _empty((N, 2 * D, 2 * H, 2 * W, Cout), a1, _act_dtype(Cout))
            wsb = nat.lib().da_upconv3d_k3_ws_bytes(N, D, H, W, Cin, Cout)
            wp, wn = _ws(wsb, a1)
            use_pack(w_tio, 0, C1, C2, Cout, N, D, H, W, 1, True)
            call_act('da_upconv3d_k3_fwd', A(a1), C1, A(a2), C2, ptr(w_tio), ptr(b), O(out), N, D, H, W, Cout, float(act_slope), wp, wn, st)
        else:
            Do, Ho, Wo = (D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1
            out = _empty((N, Do, Ho, Wo, Cout), a1, _act_dtype(Cout))
            wsb = nat.lib().da_conv3d_k3_ws_bytes(N, D, H, W, Cin, Cout, stride)
            wp, wn = _ws(wsb, a1)
            use_pack(w_tio, 0, C1, C2, Cout, N, D, H, W, stride)
            call_act('da_conv3d_k3_fwd', A(a1), C1, A(a2), C2, ptr(w_tio), ptr(b), O(out),
                     N, D, H, W, Cout, stride, float(act_slope), wp, wn, st)
        ctx.dims = (N, D, H, W, C1, C2, Cout, stride, float(act_slope), wsb)
        ctx.has_bias = bias is not None
        ctx.wparam, ctx.bparam = weight, bias
        ctx.save_for_backward(a1, a2, w_tio, out if act_slope >= 0 else None)
        if fork:
            return ncdhw(out), ncdhw(out.view(out.shape))
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout, *gmore):
        a1, a2, w_tio, out = ctx.saved_tensors
        N, D, H, W, C1, C2, Cout, stride, slope, wsb = ctx.dims
        up2 = ctx.up2
        st = stream()
        flops = 54.0 * (C1 + C2) * Cout * N * D * H * W * (8.0 if up2 else 1.0 / (stride ** 3))       # algorithmic (2 * 27 * Cin * Cout per output voxel)

        def k_dgrad(g_, dx1_, dx2_, wp_, wn_, st_):
            if up2:
                use_pack(w_tio, 1, C1, C2, Cout, N, D, H, W, 1, True)
                call_act('da_upconv3d_k3_dgrad', A(g_), ptr(w_tio), O(dx1_), C1, O(dx2_), C2, N, D, H, W, Cout, wp_, wn_, st_)
            else:
                use_pack(w_tio, 1, C1, C2, Cout, N, D, H, W, stride)
                call_act('da_conv3d_k3_dgrad', A(g_), ptr(w_tio), O(dx1_), C1, O(dx2_), C2, N, D, H, W, Cout, stride, wp_, wn_, st_)

        def k_wgrad(g_, dw_tio_, db_, wp_, wn_, st_):
            if up2:
                call_act('da_upconv3d_k3_wgrad', A(a1), C1, A(a2), C2, A(g_), ptr(dw_tio_), N, D, H, W, Cout, wp_, wn_, st_)
                if db_ is not None:
                    call_act('da_colsum', A(g_), g_.numel() // Cout, Cout, ptr(db_), wp_, wn_, st_)
            elif db_ is not None and (g_.dtype == torch.bfloat16 or a1.dtype == torch.bfloat16):          # (the bf16 twins leave the bias gradient to its own pass)
                call_act('da_conv3d_k3_wgrad', A(a1), C1, A(a2), C2, A(g_), ptr(dw_tio_), None, N, D, H, W, Cout, stride, wp_, wn_, st_)
                call_act('da_colsum', A(g_), g_.numel() // Cout, Cout, ptr(db_), wp_, wn_, st_)
            else:
                call_act('da_conv3d_k3_wgrad', A(a1), C1, A(a2), C2, A(g_), ptr(dw_tio_), ptr(db_), N, D, H, W, Cout, stride, wp_, wn_, st_)
        g_b = gmore[0] if (ctx.fork and gmore) else None
        if gout is None:
            gout, g_b = g_b, None
        g = ndhwc(gout)
        gb2 = ndhwc(g_b) if g_b is not None else None
        want_w = ctx.needs_input_grad[2]
        want_b = ctx.has_bias and ctx.needs_input_grad[3]
        db = None
        db_partial = None            # (partial buffer, number of partial sets): bias gradient still to be finished, on the side stream
        if out is not None or gb2 is not None:
            # dy = (g [+ g']) * act'(y) and the bias gradient (column sums of dy) in one pass
            g2 = torch.empty_like(g)
            M = g.numel() // Cout
            gbt0 = _async_target(ctx.bparam) if want_b else None
            if gbt0 is not None:
                # the per-channel finish of the column sums (a Cout-workgroup kernel) goes to the side stream and accumulates straight
                # into the flat gradient bucket: behind persistent matrix kernels such a kernel waits 20 - 100 us for a CU slot, and
                # nothing on the main stream needs its result
                pbytes = nat.lib().da_bn_ws_bytes(M, Cout)
                pbuf = torch.empty((pbytes,), dtype=torch.uint8, device=g.device)
                npar = ctypes.c_int(0)
                call_act('da_act_bwd_add_partial', A(g), A(gb2), A(out), slope if out is not None else -1.0, O(g2), M, Cout,
                         ptr(pbuf), pbytes, ctypes.byref(npar), st)
                db_partial = (pbuf, npar.value)
            else:
                db = _empty((Cout,), a1) if want_b else None
                bwp, bwn = _ws(max(wsb, nat.lib().da_bn_ws_bytes(M, Cout)), a1)
                call_act('da_act_bwd_add_dbias', A(g), A(gb2), A(out), slope if out is not None else -1.0, O(g2), ptr(db), M, Cout, bwp, bwn, st)
            g = g2
        wp, wn = _ws(wsb, a1)
        dx1 = dx2 = None
        if ctx.needs_input_grad[0] or (a2 is not None and ctx.needs_input_grad[1]):
            dx1 = torch.empty_like(a1)
            dx2 = torch.empty_like(a2) if a2 is not None else None
            _serialize_matrix_kernels(flops, N * D * H * W)
            k_dgrad(g, dx1, dx2, wp, wn, st)
        dw = None
        need_db_in_wgrad = want_b and db is None and db_partial is None
        kind_w = 'iok_flip' if ctx.transposed else 'oik'
        wt = WgradTarget(ctx.wparam, kind_w, w_tio) if want_w else _NO_WGRAD_TARGET
        gw = wt.gw
        gbt = _async_target(ctx.bparam) if want_b else None
        if db_partial is not None and not (want_w and gw is not None):
            def finish():                            # (frozen or non-bucket weight: the bias finish still goes to the side stream)
                call('da_colsum_finish', ptr(db_partial[0]), db_partial[1], Cout, ptr(gbt), 1, stream())
            _run_on_side(finish, (db_partial[0],))
            db_partial = None
        if want_w and gw is not None and (not want_b or gbt is not None):
            global _last_side_flops
            _last_side_flops = flops
            if db is not None:
                gbt.add_(db)                         # the fused pass above already produced the bias gradient (main stream)
                db = None
            # a layer whose inputs want no gradient is the net's first: nothing follows it on the main chain, while the side stream still has the weight
            # gradients of the layers before it queued up -- its own weight gradient runs on the main stream (reg step: the side stream's backlog was the step's tail)
            on_main = dx1 is None and dx2 is None
            side = torch.cuda.current_stream() if on_main else side_stream()
            if not on_main:
                side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                sst = stream()
                if db_partial is not None:
                    call('da_colsum_finish', ptr(db_partial[0]), db_partial[1], Cout, ptr(gbt), 1, sst)
                    _side_keep.append(db_partial[0])
                dbs = _empty((Cout,), a1) if need_db_in_wgrad else None
                swp, swn = _ws(max(wsb, nat.lib().da_bn_ws_bytes(g.numel() // Cout, Cout)) if up2 else wsb, a1)
                k_wgrad(g, wt.out(), dbs, swp, swn, sst)
                wt.finish()
                if dbs is not None:
                    gbt.add_(dbs)
            _side_keep.extend(t for t in (a1, a2, g) if t is not None)
        elif want_w or need_db_in_wgrad:
            dw_tio = torch.empty_like(w_tio)
            dbw = _empty((Cout,), a1) if need_db_in_wgrad else None
            if up2 and dbw is not None:
                wp, wn = _ws(max(wsb, nat.lib().da_bn_ws_bytes(g.numel() // Cout, Cout)), a1)
            k_wgrad(g, dw_tio, dbw, wp, wn, st)
            if dbw is not None:
                db = dbw
            if want_w:
                dw = grad_for_autograd(dw_tio, kind_w, ctx.wparam)
        return (ncdhw(dx1) if dx1 is not None else None, ncdhw(dx2) if dx2 is not None else None, dw, db, None, None) + (None,) * ctx.n_extra


def upconv_supported(C1, C2, Cout):
    """Can `conv3x3x3(F.interpolate(cat(x1, x2), scale 2, nearest))` run with the up-sampling folded in (conv3d_up2.hip)?  Channel counts
    as da_upconv3d_k3_supported documents; only in split matrix mode (the kernels' arithmetic)."""
    return bool(nat.lib().da_upconv3d_k3_supported(int(C1), int(C2), int(Cout)))


class Conv1x1Fn(Function):
    """nn.Conv3d(Cin, Cout, 1): the segmentation head (unets.py:249-250)."""

    @staticmethod
    def forward(ctx, x, weight, bias, *extra):
        pro = extra[0] if extra else None          # (scale, shift, slope) still to be applied to x (LazyAct input)
        ctx.n_extra = len(extra)
        a = ndhwc(x)
        N, D, H, W, Cin = a.shape
        Cout = weight.shape[0]
        st = stream()
        w_io = weight_tio(weight, 'oik').view(Cin, Cout)
        out = _empty((N, D, H, W, Cout), a)
        M = N * D * H * W
        b = bias.detach().contiguous() if bias is not None else None
        wp, wn = _ws(nat.lib().da_pointwise_ws_bytes(1, Cin, Cout), a)
        if pro is not None and not call_act('da_conv1x1_fwd_pro', A(a), ptr(pro[0]), ptr(pro[1]), float(pro[2]), ptr(w_io), ptr(b), O(out),
                                            M, Cin, Cout, wp, wn, st, may_decline=True):
            a, pro = _apply_pro(a, pro, st), None
        if pro is None:
            call_act('da_conv1x1_fwd', A(a), ptr(w_io), ptr(b), O(out), M, Cin, Cout, wp, wn, st)
        ctx.has_bias = bias is not None
        ctx.wparam = weight
        ctx.pro_slope = pro[2] if pro is not None else None
        ctx.save_for_backward(a, w_io, pro[0] if pro is not None else None, pro[1] if pro is not None else None)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        a, w_io, ps, pt = ctx.saved_tensors
        Cin, Cout = w_io.shape
        M = a.numel() // Cin
        st = stream()
        g = ndhwc(gout)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(a)
            wp, wn = _ws(nat.lib().da_pointwise_ws_bytes(1, Cin, Cout), a)
            call_act('da_conv1x1_dgrad', A(g), ptr(w_io), O(dx), M, Cin, Cout, wp, wn, st)
        # (the head's weight gradient stays on the main stream: it is the first backward kernel, HBM-bound like its neighbours --
        # on the side stream it only competed with them: 39.2 -> 41.5 ms)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw_io = torch.empty_like(w_io)
            db = _empty((Cout,), a) if ctx.has_bias else None
            wp, wn = _ws(nat.lib().da_conv1x1_wgrad_ws_bytes(M, Cin, Cout), a)
            if ps is not None:
                if not call_act('da_conv1x1_wgrad_pro', A(a), ptr(ps), ptr(pt), float(ctx.pro_slope), A(g), ptr(dw_io), ptr(db),
                                M, Cin, Cout, wp, wn, st, may_decline=True):
                    call_act('da_conv1x1_wgrad', A(_apply_pro(a, (ps, pt, ctx.pro_slope), st)), A(g), ptr(dw_io), ptr(db), M, Cin, Cout, wp, wn, st)
            else:
                call_act('da_conv1x1_wgrad', A(a), A(g), ptr(dw_io), ptr(db), M, Cin, Cout, wp, wn, st)
            dw = grad_for_autograd(dw_io.view(1, Cin, Cout), 'oik', ctx.wparam)
        return ((ncdhw(dx) if dx is not None else None), dw, db) + (None,) * ctx.n_extra


class DeconvK2S2Fn(Function):
    """nn.ConvTranspose3d(k=2, s=2) (unets.py:49,55)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        a = ndhwc(x)
        N, D, H, W, Cin = a.shape
        Cout = weight.shape[1]
        if weight.shape[0] != Cin or tuple(weight.shape[2:]) != (2, 2, 2):
            raise ValueError('ConvTranspose3d weight %s does not match input channels %d' % (tuple(weight.shape), Cin))
        st = stream()
        w_tio = weight_tio(weight, 'iok')
        out = _empty((N, 2 * D, 2 * H, 2 * W, Cout), a, _act_dtype(Cout))
        b = bias.detach().contiguous() if bias is not None else None
        wp, wn = _ws(nat.lib().da_pointwise_ws_bytes(8, Cin, Cout), a)
        call_act('da_deconv_k2s2_fwd', A(a), ptr(w_tio), ptr(b), O(out), N, D, H, W, Cin, Cout, wp, wn, st)
        ctx.has_bias = bias is not None
        ctx.wparam = weight
        ctx.save_for_backward(a, w_tio)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        a, w_tio = ctx.saved_tensors
        N, D, H, W, Cin = a.shape
        Cout = w_tio.shape[2]
        st = stream()
        g = ndhwc(gout)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(a)
            wp, wn = _ws(nat.lib().da_pointwise_ws_bytes(8, Cin, Cout), a)
            call_act('da_deconv_k2s2_dgrad', A(g), ptr(w_tio), O(dx), N, D, H, W, Cin, Cout, wp, wn, st)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw_tio = torch.empty_like(w_tio)
            db = _empty((Cout,), a) if ctx.has_bias else None
            wp, wn = _ws(nat.lib().da_deconv_k2s2_wgrad_ws_bytes(N, D, H, W, Cin, Cout), a)
            call_act('da_deconv_k2s2_wgrad', A(a), A(g), ptr(dw_tio), ptr(db), N, D, H, W, Cin, Cout, wp, wn, st)
            dw = grad_for_autograd(dw_tio, 'iok', ctx.wparam)
        return (ncdhw(dx) if dx is not None else None), dw, db


class ConvK2S2Fn(Function):
    """nn.Conv3d(kernel 2, stride 2, padding 0): UNet_generator(maxpool=False) down-sampler (unets.py:231-233).  The adjoint of
    the k2/s2 transposed conv, on the same pointwise MFMA kernels.  Even spatial sizes, channels in multiples of 16."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        a = ndhwc(x)
        N, D2, H2, W2, Cin = a.shape
        Cout = weight.shape[0]
        if weight.shape[1] != Cin or tuple(weight.shape[2:]) != (2, 2, 2):
            raise ValueError('Conv3d(k2,s2) weight %s does not match input channels %d' % (tuple(weight.shape), Cin))
        if (D2 | H2 | W2) & 1 or Cin % 16 or Cout % 16:
            raise NotImplementedError('HIP strided-conv down-sampler: even spatial sizes and channels in multiples of 16')
        D, H, W = D2 // 2, H2 // 2, W2 // 2
        st = stream()
        w_tio = weight_tio(weight, 'oik')
        out = _empty((N, D, H, W, Cout), a, _act_dtype(Cout))
        b = bias.detach().contiguous() if bias is not None else None
        wp, wn = _ws(nat.lib().da_pointwise_ws_bytes(8, Cin, Cout), a)
        call_act('da_conv_k2s2_fwd', A(a), ptr(w_tio), ptr(b), O(out), N, D, H, W, Cin, Cout, wp, wn, st)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(a, w_tio)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        a, w_tio = ctx.saved_tensors
        N, D2, H2, W2, Cin = a.shape
        D, H, W = D2 // 2, H2 // 2, W2 // 2
        Cout = w_tio.shape[2]
        st = stream()
        g = ndhwc(gout)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(a)
            wp, wn = _ws(nat.lib().da_pointwise_ws_bytes(8, Cout, Cin), a)
            call_act('da_conv_k2s2_dgrad', A(g), ptr(w_tio), O(dx), N, D, H, W, Cin, Cout, wp, wn, st)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw_toi = _empty((8, Cout, Cin), a)
            db = _empty((Cout,), a) if ctx.has_bias else None
            wp, wn = _ws(nat.lib().da_conv_k2s2_wgrad_ws_bytes(N, D, H, W, Cin, Cout), a)
            call_act('da_conv_k2s2_wgrad', A(a), A(g), ptr(dw_toi), ptr(db), N, D, H, W, Cin, Cout, wp, wn, st)
            dw = _empty((Cout, Cin, 2, 2, 2), a)
            call('da_w_tio_to_iok', ptr(dw_toi), ptr(dw), Cout, Cin, 8, st)          # [8][Cout][Cin] -> [Cout][Cin][8]
        return (ncdhw(dx) if dx is not None else None), dw, db


class UpsampleTrilinear2Fn(Function):
    """nn.Upsample(scale_factor=2, mode='trilinear') (align_corners=False): UNet_generator(upsample=True), unets.py:236."""

    @staticmethod
    def forward(ctx, x):
        a = ndhwc(x)
        N, D, H, W, C = a.shape
        out = _empty((N, 2 * D, 2 * H, 2 * W, C), a, a.dtype)
        call_act('da_upsample_trilinear2_fwd', A(a), O(out), N, D, H, W, C, stream())
        ctx.dims = (N, D, H, W, C)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        N, D, H, W, C = ctx.dims
        g = ndhwc(gout)
        dx = _empty((N, D, H, W, C), g, g.dtype)
        call_act('da_upsample_trilinear2_bwd', A(g), O(dx), N, D, H, W, C, stream())
        return ncdhw(dx)


# ------------------------------------------------------------------------------------------------
# BatchNorm3d + activation
# ------------------------------------------------------------------------------------------------
class BNActFn(Function):
    """nn.BatchNorm3d followed by LeakyReLU/ReLU (unets.py:31-32,51-52), one fused pass each way.
    running_mean / running_var are updated in place in training mode (momentum, unbiased variance)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, training, momentum, eps, slope):
        a = ndhwc(y)
        C = a.shape[-1]
        M = a.numel() // C
        st = stream()
        stats = _empty((4, C), a)                     # mean, rstd, scale, shift
        g = gamma.detach().contiguous() if gamma is not None else None
        b = beta.detach().contiguous() if beta is not None else None
        wsb = nat.lib().da_bn_ws_bytes(M, C)
        if training or running_mean is None:
            wp, wn = _ws(wsb, a)
            call_act('da_bn_train_stats', A(a), M, C, ptr(g), ptr(b), float(eps), float(momentum),
                     ptr(running_mean), ptr(running_var), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), wp, wn, st)
        else:
            call('da_bn_eval_affine', ptr(g), ptr(b), ptr(running_mean), ptr(running_var), float(eps), C,
                 ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), st)
        out = torch.empty_like(a)
        call_act('da_bn_act_fwd', A(a), ptr(stats[2]), ptr(stats[3]), float(slope), O(out), M, C, st)
        ctx.cfg = (M, C, float(slope), bool(training or running_mean is None), wsb)
        ctx.save_for_backward(a, stats, g)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        a, stats, g = ctx.saved_tensors
        M, C, slope, train, wsb = ctx.cfg
        st = stream()
        go = ndhwc(gout)
        dx = torch.empty_like(a)
        dgb = _empty((2, C), a)
        wp, wn = _ws(wsb, a)
        call_act('da_bn_act_bwd', A(go), A(a), ptr(stats[0]), ptr(stats[1]), ptr(g), ptr(stats[2]), ptr(stats[3]),
                 slope, 1 if train else 0, O(dx), ptr(dgb[0]), ptr(dgb[1]), M, C, wp, wn, st)
        return ncdhw(dx), dgb[0], dgb[1], None, None, None, None, None, None


def _bn_forward(a, gamma, beta, running_mean, running_var, training, momentum, eps, slope, st, partials=None, apply=True):
    """stats (train: batch statistics + running-stat update, eval: running stats) and fused apply+activation.
    partials = (double tensor [nparts][2][C], nparts) when the producing conv already accumulated the sums in its epilogue."""
    C = a.shape[-1]
    M = a.numel() // C
    stats = _empty((4, C), a)                     # mean, rstd, scale, shift
    g = gamma.detach().contiguous() if gamma is not None else None
    b = beta.detach().contiguous() if beta is not None else None
    wsb = nat.lib().da_bn_ws_bytes(M, C)
    train = bool(training or running_mean is None)
    if train and partials is not None and partials[1] > 0:
        call('da_bn_train_stats_from_partials', ptr(partials[0]), partials[1], M, C, ptr(g), ptr(b), float(eps), float(momentum),
             ptr(running_mean), ptr(running_var), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), st)
    elif train:
        wp, wn = _ws(wsb, a)
        call_act('da_bn_train_stats', A(a), M, C, ptr(g), ptr(b), float(eps), float(momentum),
                 ptr(running_mean), ptr(running_var), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), wp, wn, st)
    else:
        call('da_bn_eval_affine', ptr(g), ptr(b), ptr(running_mean), ptr(running_var), float(eps), C,
             ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), st)
    out = None
    if apply:
        out = torch.empty_like(a)
        call_act('da_bn_act_fwd', A(a), ptr(stats[2]), ptr(stats[3]), float(slope), O(out), M, C, st)
    return out, stats, g, (M, C, float(slope), train, wsb)


# BatchNorm-backward sums that the PRODUCER of a gradient tensor accumulated in its own epilogue (da_head_dice_bwd_bst): gradient data pointer ->
# (the gradient tensor itself -- kept alive so that the pointer cannot be reused while the entry exists --, partials, count, M, C).  The consumer
# (_bn_backward of the layer whose output that gradient belongs to) pops its entry; FlatAdam.zero_grad / step drop whatever was never consumed.
_bwd_stats = {}
# one-input layers whose data gradient carries the producer's sums: <= 16 input channels.  The entry also takes 32 (two N-tiles, one per workgroup), measured
# slower in the step: 20.46 - 20.56 -> 20.59 - 20.67 ms.  The 32 + 16 concat layer's data gradient also carries them (reached with LAZY_BN_UPSAMPLER only).
_DGRAD_BST_MAXC = 16
FUSE_BN_BWD_STATS = True        # (tests: False takes every BatchNorm-backward sum by the stand-alone pass)


def drop_bwd_stats(*_):
    _bwd_stats.clear()


def _direct_small_target(small_params, C, want_dbias):
    """The (3, C) slice of a FlatAdam gradient bucket that holds (bias, gamma, beta) of one block, if the BatchNorm-backward kernels may WRITE their three
    results straight into it: all three gradients are views of a registered bucket, consecutive there (conv.bias, BN.weight, BN.bias are consecutive
    parameters), and still all zeros since zero_grad (`_da_gz`, the mark the direct weight gradients use).  Saves the (3, C) scratch tensor and one
    torch add per block (19 launches on the dependent chain of a seg step).  None: take the scratch tensor + _accumulate_small_grads."""
    if small_params is None or not want_dbias:
        return None
    bias, gamma, beta = small_params
    if bias is None or gamma is None or beta is None:
        return None
    if not (getattr(bias, '_da_gz', False) and getattr(gamma, '_da_gz', False) and getattr(beta, '_da_gz', False)):
        return None
    gb, gg, gbt = _async_target(bias), _async_target(gamma), _async_target(beta)
    if gb is None or gg is None or gbt is None:
        return None
    if not (gb.numel() == gg.numel() == gbt.numel() == C and gb.is_contiguous() and gg.data_ptr() == gb.data_ptr() + 4 * C and gbt.data_ptr() == gg.data_ptr() + 4 * C):
        return None
    bias._da_gz = gamma._da_gz = beta._da_gz = False
    return torch.as_strided(gb, (3, C), (C, 1))


def _bn_backward(go, y, stats, cfg, want_dbias, st, small_params=None):
    """BN+activation backward; returns (dy, dgamma, dbeta, dbias_of_producer or None) -- the producer's bias gradient is the
    column sum of dy and is accumulated inside the apply pass.  With `small_params` = the block's (bias, gamma, beta) parameters the three
    gradients may be written straight into the optimiser's bucket (_direct_small_target); the returned gradients are then all None."""
    M, C, slope, train, wsb = cfg
    dy = torch.empty_like(y)
    direct = _direct_small_target(small_params, C, want_dbias) if train else None
    dgb = direct if direct is not None else _empty((3, C), y)                   # rows: producer bias, gamma, beta -- the order the parameters have in a block
    wp, wn = _ws(wsb, y)
    pre = _bwd_stats.pop(go.data_ptr(), None) if _bwd_stats else None
    if pre is not None and train and pre[3] == M and pre[4] == C and go.dtype == torch.float32 and y.dtype == torch.float32 and go.is_contiguous():
        call('da_bn_act_bwd_dbias_pre', ptr(go), ptr(y), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]),
             slope, 1, ptr(dy), ptr(dgb[1]), ptr(dgb[2]), ptr(dgb[0]) if want_dbias else None, M, C, ptr(pre[1]), pre[2], wp, wn, st)
        return (dy, None, None, None) if direct is not None else (dy, dgb[1], dgb[2], (dgb[0] if want_dbias else None))
    call_act('da_bn_act_bwd_dbias', A(go), A(y), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]),
             slope, 1 if train else 0, O(dy), ptr(dgb[1]), ptr(dgb[2]), ptr(dgb[0]) if want_dbias else None, M, C, wp, wn, st)
    return (dy, None, None, None) if direct is not None else (dy, dgb[1], dgb[2], (dgb[0] if want_dbias else None))


def _accumulate_small_grads(bias, gamma, beta, db, dgamma, dbeta):
    """With ASYNC_WGRAD (gradients may be accumulated straight into FlatAdam's bucket): if bias / gamma / beta of a block sit next to
    each other in the bucket (they do: conv.bias, BN.weight, BN.bias are consecutive parameters) their three gradients -- one (3, C)
    tensor, see _bn_backward -- are added with ONE kernel instead of three autograd accumulations.  Returns the gradients still to
    be handed to autograd (None where already accumulated)."""
    if db is None or dgamma is None or dbeta is None:
        return db, dgamma, dbeta
    gb, gg, gbt = _async_target(bias), _async_target(gamma), _async_target(beta)
    if gb is None or gg is None or gbt is None:
        return db, dgamma, dbeta
    C = db.numel()
    if not (gb.numel() == gg.numel() == gbt.numel() == C and gg.data_ptr() == gb.data_ptr() + 4 * C and gbt.data_ptr() == gg.data_ptr() + 4 * C
            and dgamma.data_ptr() == db.data_ptr() + 4 * C and dbeta.data_ptr() == dgamma.data_ptr() + 4 * C):
        return db, dgamma, dbeta
    dst = torch.as_strided(gb, (3 * C,), (1,))
    src = torch.as_strided(db, (3 * C,), (1,))
    dst.add_(src)
    return None, None, None


def _wgrad_with_pro(a1, C1, pro1, a2, C2, pro2, dy, dw_tio, N, D, H, W, Cout, wp, wn, st):
    """3x3x3 weight gradient whose inputs may still carry a deferred BatchNorm + activation."""
    if pro1 is not None or pro2 is not None:
        s1, t1, sl1 = _pro_args(pro1)
        s2, t2, sl2 = _pro_args(pro2)
        if call_act('da_conv3d_k3_wgrad_pro', A(a1), C1, s1, t1, sl1, A(a2), C2, s2, t2, sl2, A(dy), ptr(dw_tio),
                    N, D, H, W, Cout, wp, wn, st, may_decline=True):
            return
        a1 = _apply_pro(a1, pro1, st)
        a2 = _apply_pro(a2, pro2, st) if a2 is not None else None
    call_act('da_conv3d_k3_wgrad', A(a1), C1, A(a2), C2, A(dy), ptr(dw_tio), None, N, D, H, W, Cout, 1, wp, wn, st)


class ConvBNActFn(Function):
    """unets.convBlock with batchnorm=True as ONE autograd node: Conv3d(k3,p1) on concat(x1, x2) -> BatchNorm3d -> LeakyReLU
    (unets.py:24-33).  Saves the raw conv output; the backward runs BN/act backward (which also yields the conv bias gradient),
    then the conv data / weight gradients."""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, gamma, beta, running_mean, running_var, training, momentum, eps, slope, *extra):
        transposed = bool(extra[0]) if extra else False        # ConvTranspose3d(k3,s1,p1) weight, see Conv3dK3Fn
        # extra[1] / extra[2]: (scale, shift, slope) still to be applied to x1 / x2 (LazyAct inputs); extra[3]: return the raw output
        # + (scale, shift) instead of the activated tensor (LazyAct output)
        pro1 = extra[1] if len(extra) > 1 else None
        pro2 = extra[2] if len(extra) > 2 else None
        lazy_out = bool(extra[3]) if len(extra) > 3 else False
        ctx.n_extra, ctx.transposed, ctx.lazy_out = len(extra), transposed, lazy_out
        a1 = ndhwc(x1)
        a2 = ndhwc(x2) if x2 is not None else None
        N, D, H, W, C1 = a1.shape
        C2 = a2.shape[-1] if a2 is not None else 0
        Cout, Cin = (weight.shape[1], weight.shape[0]) if transposed else (weight.shape[0], weight.shape[1])
        if Cin != C1 + C2 or tuple(weight.shape[2:]) != (3, 3, 3):
            raise ValueError('weight %s does not match input channels %d+%d' % (tuple(weight.shape), C1, C2))
        st = stream()
        w_tio = weight_tio(weight, 'iok_flip' if transposed else 'oik')
        y = _empty((N, D, H, W, Cout), a1, _act_dtype(Cout))
        wsb = nat.lib().da_conv3d_k3_ws_bytes(N, D, H, W, Cin, Cout, 1)
        wp, wn = _ws(wsb, a1)
        b = bias.detach().contiguous() if bias is not None else None
        partials = None
        train_stats = bool(training or running_mean is None)
        pbuf = torch.empty((512, 2, Cout), dtype=torch.float64, device=a1.device) if train_stats else None
        npar = ctypes.c_int(0)
        cap = 512 if train_stats else 0
        done = False
        if pro1 is not None or pro2 is not None:
            s1, t1, sl1 = _pro_args(pro1)
            s2, t2, sl2 = _pro_args(pro2)
            use_pack(w_tio, 0, C1, C2, Cout, N, D, H, W)
            done = call_act('da_conv3d_k3_fwd_pro', A(a1), C1, s1, t1, sl1, A(a2), C2, s2, t2, sl2, ptr(w_tio), ptr(b), O(y),
                            N, D, H, W, Cout, -1.0, ptr(pbuf), cap, ctypes.byref(npar), wp, wn, st, may_decline=True)
            if not done:           # shape not taken by the prologue kernels: apply the deferred activation as its own pass
                a1, a2, pro1, pro2 = _apply_pro(a1, pro1, st), (_apply_pro(a2, pro2, st) if a2 is not None else None), None, None
        if not done:
            use_pack(w_tio, 0, C1, C2, Cout, N, D, H, W)
            if train_stats:
                # the MFMA epilogue accumulates the BatchNorm partial sums, so the statistics need no pass over y
                call_act('da_conv3d_k3_fwd_bnstats', A(a1), C1, A(a2), C2, ptr(w_tio), ptr(b), O(y), N, D, H, W, Cout, 1,
                         ptr(pbuf), cap, ctypes.byref(npar), wp, wn, st)
            else:
                call_act('da_conv3d_k3_fwd', A(a1), C1, A(a2), C2, ptr(w_tio), ptr(b), O(y), N, D, H, W, Cout, 1, -1.0, wp, wn, st)
        if train_stats:
            partials = (pbuf, npar.value)
        out, stats, g, cfg = _bn_forward(y, gamma, beta, running_mean, running_var, training, momentum, eps, slope, st, partials,
                                         apply=not lazy_out)
        ctx.dims = (N, D, H, W, C1, C2, Cout, wsb)
        ctx.cfg = cfg
        ctx.has_bias = bias is not None
        ctx.wparam = weight
        ctx.small_params = (bias, gamma, beta)
        ctx.pro_slopes = (pro1[2] if pro1 is not None else None, pro2[2] if pro2 is not None else None)
        ctx.save_for_backward(a1, a2, w_tio, y, stats, pro1[0] if pro1 is not None else None, pro1[1] if pro1 is not None else None,
                              pro2[0] if pro2 is not None else None, pro2[1] if pro2 is not None else None)
        if lazy_out:
            scale, shift = stats[2], stats[3]
            ctx.mark_non_differentiable(scale, shift)
            ctx.set_materialize_grads(False)          # no zero-filled gradients for (scale, shift): they are statistics, not graph nodes
            return ncdhw(y), scale, shift
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout, *unused):
        a1, a2, w_tio, y, stats, p1s, p1t, p2s, p2t = ctx.saved_tensors
        pro1 = (p1s, p1t, ctx.pro_slopes[0]) if p1s is not None else None
        pro2 = (p2s, p2t, ctx.pro_slopes[1]) if p2s is not None else None
        N, D, H, W, C1, C2, Cout, wsb = ctx.dims
        st = stream()
        dy, dgamma, dbeta, db = _bn_backward(ndhwc(gout), y, stats, ctx.cfg, ctx.has_bias, st, ctx.small_params)
        wp, wn = _ws(wsb, a1)
        dx1 = dx2 = None
        if ctx.needs_input_grad[0] or (a2 is not None and ctx.needs_input_grad[1]):
            dx1 = torch.empty_like(a1)
            dx2 = torch.empty_like(a2) if a2 is not None else None
            _serialize_matrix_kernels(54.0 * (C1 + C2) * Cout * N * D * H * W, N * D * H * W)
            use_pack(w_tio, 1, C1, C2, Cout, N, D, H, W)
            done = False
            if (FUSE_BN_BWD_STATS and pro1 is not None and ((a2 is None and C1 <= _DGRAD_BST_MAXC) or (a2 is not None and C1 == 32 and C2 == 16 and a2.dtype == torch.float32))
                    and _matrix_mode == 'fp32_split' and dy.dtype == torch.float32
                    and a1.dtype == torch.float32 and p1s.data_ptr() - 8 * C1 == p1t.data_ptr() - 12 * C1 and p1s.untyped_storage().data_ptr() <= p1s.data_ptr() - 8 * C1):
                # (also while a HIP graph is being captured: whether the route exists is decided on the host, and a graphed step must run the same kernels --
                # the same summation order -- as an eager one: tests/test_gpu_dp.py compares them bit for bit)
                # the input was the raw output of a conv + BatchNorm block (a1) with its statistics rows (mean, rstd, scale, shift): that block's
                # BatchNorm-backward sums are accumulated in this data gradient's epilogue instead of a pass over (dx1, a1)
                bst = torch.empty((512, 2, C1), dtype=torch.float64, device=a1.device)
                nb = ctypes.c_int(0)
                done = nat.call_supported('da_conv3d_k3_dgrad_bst', ptr(dy), ptr(w_tio), ptr(dx1), C1, ptr(dx2), C2, N, D, H, W, Cout, ptr(a1), ctypes.c_void_p(p1s.data_ptr() - 8 * C1),
                                          float(ctx.pro_slopes[0]), ptr(bst), 512, ctypes.byref(nb), wp, wn, st) and nb.value > 0
                if done:
                    _bwd_stats[dx1.data_ptr()] = (dx1, bst, nb.value, N * D * H * W, C1)
                else:
                    use_pack(w_tio, 1, C1, C2, Cout, N, D, H, W)          # (the hand-over was dropped with the declined call)
            if not done:
                call_act('da_conv3d_k3_dgrad', A(dy), ptr(w_tio), O(dx1), C1, O(dx2), C2, N, D, H, W, Cout, 1, wp, wn, st)
        kind_w = 'iok_flip' if ctx.transposed else 'oik'
        wt = WgradTarget(ctx.wparam, kind_w, w_tio) if ctx.needs_input_grad[2] else _NO_WGRAD_TARGET
        gw = wt.gw
        if not ctx.needs_input_grad[2]:
            dw = None                                  # frozen weight: no weight-gradient kernel at all
        elif gw is not None:
            global _last_side_flops
            _last_side_flops = 54.0 * (C1 + C2) * Cout * N * D * H * W
            side = side_stream()                       # (also for the net's first layer: its weight gradient on the main stream, as in Conv3dFn.backward, gained nothing here)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                sst = stream()
                swp, swn = _ws(wsb, a1)
                _wgrad_with_pro(a1, C1, pro1, a2, C2, pro2, dy, wt.out(), N, D, H, W, Cout, swp, swn, sst)
                wt.finish()
            _side_keep.extend(t for t in (a1, a2, dy, p1s, p1t, p2s, p2t) if t is not None)
            dw = None
        else:
            dw_tio = torch.empty_like(w_tio)
            _wgrad_with_pro(a1, C1, pro1, a2, C2, pro2, dy, dw_tio, N, D, H, W, Cout, wp, wn, st)
            dw = grad_for_autograd(dw_tio, kind_w, ctx.wparam)
        db, dgamma, dbeta = _accumulate_small_grads(*ctx.small_params, db, dgamma, dbeta)
        return (ncdhw(dx1) if dx1 is not None else None, ncdhw(dx2) if dx2 is not None else None, dw, db, dgamma, dbeta,
                None, None, None, None, None, None) + (None,) * ctx.n_extra


FUSE_DECONV_BN_BWD = True      # (tests: False runs the up-sampler block's backward as three calls)


def _deconv_bn_bwd_fused(ctx, go, a, w_tio, y, stats, N, D, H, W, Cin, Cout, st):
    """The up-sampler block's whole backward as ONE pass over (gout, y) (da_deconv_k2s2_bn_bwd: BatchNorm-backward apply on the fly + transposed-conv data
    and weight gradient; the tensor dy is never written).  Taken in training mode, fp32 tensors, Cin = Cout = 32 (the full-resolution link of UNet_light),
    when input and weight both want their gradients and the weight gradient goes straight into the optimiser's bucket or to a fresh tensor.  Runs on the
    MAIN stream (it replaces the apply pass and the data gradient as well; the side stream keeps the 3x3x3 weight gradients).  None: not taken."""
    M, C, slope, train, wsb = ctx.cfg
    if not (FUSE_DECONV_BN_BWD and train and Cin == 32 and Cout == 32 and go.dtype == torch.float32 and y.dtype == torch.float32 and a.dtype == torch.float32
            and go.is_contiguous() and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and ctx.has_bias):
        return None
    pre = _bwd_stats.pop(go.data_ptr(), None) if _bwd_stats else None
    if pre is not None and not (pre[3] == M and pre[4] == C):
        pre = None
    dx = torch.empty_like(a)
    direct = _direct_small_target(ctx.small_params, C, True)
    dgb = direct if direct is not None else _empty((3, C), y)         # rows: transposed-conv bias, gamma, beta
    wt = WgradTarget(ctx.wparam, 'iok', w_tio)
    wp, wn = _ws(nat.lib().da_deconv_k2s2_bn_bwd_ws_bytes(N, D, H, W, Cin, Cout), a)
    # (the weight-gradient target: the optimiser's bucket slice / a scratch tensor added into it by wt.finish(), or a fresh tensor handed to autograd)
    if wt.gw is not None:
        dw_out = wt.out()
    else:
        dw_out = torch.empty_like(w_tio)
    ok = nat.call_supported('da_deconv_k2s2_bn_bwd', ptr(go), ptr(y), ptr(stats[0]), ptr(stats[1]), ptr(stats[2]), ptr(stats[3]), float(slope),
                            ptr(a), ptr(w_tio), ptr(dx), ptr(dw_out), ptr(dgb[0]), ptr(dgb[1]), ptr(dgb[2]),
                            N, D, H, W, Cin, Cout, ptr(pre[1]) if pre is not None else None, pre[2] if pre is not None else 0, wp, wn, st)
    if not ok:
        raise nat.NativeError('da_deconv_k2s2_bn_bwd declined a shape da_deconv_bn_bwd_supported accepts')
    if wt.gw is not None:
        wt.finish()
        dw = None
    else:
        dw = grad_for_autograd(dw_out, 'iok', ctx.wparam)
    if direct is not None:
        db = dgamma = dbeta = None
    else:
        db, dgamma, dbeta = _accumulate_small_grads(*ctx.small_params, dgb[0], dgb[1], dgb[2])
    return (ncdhw(dx), dw, db, dgamma, dbeta, None, None, None, None, None, None) + (None,) * ctx.n_extra


class DeconvBNActFn(Function):
    """unets.deconvBlock with batchnorm=True as one autograd node: ConvTranspose3d(k2,s2) -> BatchNorm3d -> LeakyReLU (unets.py:42-52)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, training, momentum, eps, slope, *extra):
        lazy_out = bool(extra[0]) if extra else False            # return the raw output + (scale, shift): see LazyAct
        ctx.n_extra = len(extra)
        a = ndhwc(x)
        N, D, H, W, Cin = a.shape
        Cout = weight.shape[1]
        if weight.shape[0] != Cin or tuple(weight.shape[2:]) != (2, 2, 2):
            raise ValueError('ConvTranspose3d weight %s does not match input channels %d' % (tuple(weight.shape), Cin))
        st = stream()
        w_tio = weight_tio(weight, 'iok')
        y = _empty((N, 2 * D, 2 * H, 2 * W, Cout), a, _act_dtype(Cout))
        b = bias.detach().contiguous() if bias is not None else None
        wp, wn = _ws(nat.lib().da_pointwise_ws_bytes(8, Cin, Cout), a)
        partials = None
        if training or running_mean is None:
            # the matrix-core epilogue accumulates the BatchNorm partial sums (one set per 256 coarse voxels): no statistics pass over y
            nblk = (N * D * H * W + 255) // 256
            pbuf = torch.empty((nblk, 2, Cout), dtype=torch.float64, device=a.device)
            npar = ctypes.c_int(0)
            call_act('da_deconv_k2s2_fwd_bnstats', A(a), ptr(w_tio), ptr(b), O(y), N, D, H, W, Cin, Cout, ptr(pbuf), nblk, ctypes.byref(npar), wp, wn, st)
            partials = (pbuf, npar.value)
        else:
            call_act('da_deconv_k2s2_fwd', A(a), ptr(w_tio), ptr(b), O(y), N, D, H, W, Cin, Cout, wp, wn, st)
        out, stats, g, cfg = _bn_forward(y, gamma, beta, running_mean, running_var, training, momentum, eps, slope, st, partials, apply=not lazy_out)
        ctx.cfg = cfg
        ctx.has_bias = bias is not None
        ctx.wparam = weight
        ctx.small_params = (bias, gamma, beta)
        ctx.save_for_backward(a, w_tio, y, stats)
        if lazy_out:
            scale, shift = stats[2], stats[3]
            ctx.mark_non_differentiable(scale, shift)
            ctx.set_materialize_grads(False)          # no zero-filled gradients for (scale, shift): they are statistics, not graph nodes
            return ncdhw(y), scale, shift
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout, *unused):
        a, w_tio, y, stats = ctx.saved_tensors
        N, D, H, W, Cin = a.shape
        Cout = w_tio.shape[2]
        st = stream()
        fused = _deconv_bn_bwd_fused(ctx, ndhwc(gout), a, w_tio, y, stats, N, D, H, W, Cin, Cout, st)
        if fused is not None:
            return fused
        dy, dgamma, dbeta, db = _bn_backward(ndhwc(gout), y, stats, ctx.cfg, ctx.has_bias, st, ctx.small_params)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(a)
            wp, wn = _ws(nat.lib().da_pointwise_ws_bytes(8, Cin, Cout), a)
            call_act('da_deconv_k2s2_dgrad', A(dy), ptr(w_tio), O(dx), N, D, H, W, Cin, Cout, wp, wn, st)
        wt = WgradTarget(ctx.wparam, 'iok', w_tio) if ctx.needs_input_grad[1] else _NO_WGRAD_TARGET
        gw = wt.gw
        if not ctx.needs_input_grad[1]:
            dw = None                                  # frozen weight
        elif gw is not None:
            def side_work():                        # HBM-bound: overlaps the MFMA-bound conv data gradients on the main stream
                swp, swn = _ws(nat.lib().da_deconv_k2s2_wgrad_ws_bytes(N, D, H, W, Cin, Cout), a)
                call_act('da_deconv_k2s2_wgrad', A(a), A(dy), ptr(wt.out()), None, N, D, H, W, Cin, Cout, swp, swn, stream())
                wt.finish()
            _run_on_side(side_work, (a, dy))
            dw = None
        else:
            dw_tio = torch.empty_like(w_tio)
            wp, wn = _ws(nat.lib().da_deconv_k2s2_wgrad_ws_bytes(N, D, H, W, Cin, Cout), a)
            call_act('da_deconv_k2s2_wgrad', A(a), A(dy), ptr(dw_tio), None, N, D, H, W, Cin, Cout, wp, wn, st)
            dw = grad_for_autograd(dw_tio, 'iok', ctx.wparam)
        db, dgamma, dbeta = _accumulate_small_grads(*ctx.small_params, db, dgamma, dbeta)
        return ((ncdhw(dx) if dx is not None else None), dw, db, dgamma, dbeta, None, None, None, None, None, None) + (None,) * ctx.n_extra


class ActFn(Function):
    """Stand-alone ReLU / LeakyReLU (used when a block has no BatchNorm and the conv did not fuse it)."""

    @staticmethod
    def forward(ctx, x, slope):
        a = ndhwc(x)
        C = a.shape[-1]
        ones = torch.ones(C, dtype=torch.float32, device=a.device)
        zeros = torch.zeros(C, dtype=torch.float32, device=a.device)
        out = torch.empty_like(a)
        call_act('da_bn_act_fwd', A(a), ptr(ones), ptr(zeros), float(slope), O(out), a.numel() // C, C, stream())
        ctx.slope = float(slope)
        ctx.save_for_backward(out)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        out, = ctx.saved_tensors
        g = ndhwc(gout)
        dx = torch.empty_like(out)
        call_act('da_act_bwd', A(g), A(out), ctx.slope, O(dx), g.numel(), stream())
        return ncdhw(dx), None


# ------------------------------------------------------------------------------------------------
# pooling / resampling
# ------------------------------------------------------------------------------------------------
class MaxPool2Fn(Function):
    """nn.MaxPool3d(2) (unets.py:230,267)."""

    @staticmethod
    def forward(ctx, x):
        a = ndhwc(x)
        N, D, H, W, C = a.shape
        out = _empty((N, D // 2, H // 2, W // 2, C), a, a.dtype)
        call_act('da_maxpool2_fwd', A(a), O(out), N, D, H, W, C, stream())
        ctx.save_for_backward(a)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        a, = ctx.saved_tensors
        N, D, H, W, C = a.shape
        g = ndhwc(gout)
        dx = torch.empty_like(a)
        call_act('da_maxpool2_bwd', A(g), A(a), O(dx), N, D, H, W, C, stream())
        return ncdhw(dx)


class MaxPool2SkipFn(Function):
    """x -> (x as the skip tensor, MaxPool3d(2)(x)) as ONE autograd node (unets.py:266-267,275): the two gradients reaching x are
    summed inside the max-pool backward kernel instead of by a separate accumulation pass."""

    @staticmethod
    def forward(ctx, x, *extra):
        # extra = (scale, shift, slope): x is a RAW producer output (LazyAct); its BatchNorm + activation is applied in the same pass that
        # pools it, and the activated tensor written by that pass is the skip tensor
        ctx.n_extra = len(extra)
        a = ndhwc(x)
        N, D, H, W, C = a.shape
        out = _empty((N, D // 2, H // 2, W // 2, C), a, a.dtype)
        st = stream()
        raw = None
        ctx.pro_slope = None
        if extra:
            act = torch.empty_like(a)
            if not call_act('da_maxpool2_fwd_pro', A(a), ptr(extra[0]), ptr(extra[1]), float(extra[2]), O(act), O(out), N, D, H, W, C, st, may_decline=True):
                act = _apply_pro(a, extra, st)
                call_act('da_maxpool2_fwd', A(act), O(out), N, D, H, W, C, st)
            ps, pt = extra[0], extra[1]
            if (FUSE_BN_BWD_STATS and a.dtype == torch.float32 and ps.data_ptr() - 8 * C == pt.data_ptr() - 12 * C
                    and ps.untyped_storage().data_ptr() <= ps.data_ptr() - 8 * C):
                # (scale, shift) are rows of the producer's [mean | rstd | scale | shift] buffer: its BatchNorm-backward sums can ride on this node's backward
                raw, ctx.pro_slope = a, float(extra[2])
            a = act
        else:
            call_act('da_maxpool2_fwd', A(a), O(out), N, D, H, W, C, st)
        if raw is not None:
            ctx.save_for_backward(a, raw, extra[0])
        else:
            ctx.save_for_backward(a)
        return ncdhw(a), ncdhw(out)

    @staticmethod
    def backward(ctx, gskip, gpool):
        a = ctx.saved_tensors[0]
        N, D, H, W, C = a.shape
        if gpool is None:
            return (gskip,) + (None,) * ctx.n_extra
        g = ndhwc(gpool)
        dx = torch.empty_like(a)
        if len(ctx.saved_tensors) == 3 and FUSE_BN_BWD_STATS and g.dtype == torch.float32:
            # the pooled tensor was the raw output of a conv + BatchNorm block: dx and that block's BatchNorm-backward sums from one kernel
            raw, ps = ctx.saved_tensors[1], ctx.saved_tensors[2]
            bst = torch.empty((1024, 2, C), dtype=torch.float64, device=a.device)
            nb = ctypes.c_int(0)
            gs = ndhwc(gskip) if gskip is not None else None
            if nat.call_supported('da_maxpool2_bwd_bst', ptr(g), ptr(raw), ptr(gs), ptr(dx), N, D, H, W, C, ctypes.c_void_p(ps.data_ptr() - 8 * C),
                                  ctx.pro_slope, ptr(bst), 1024, ctypes.byref(nb), stream()) and nb.value > 0:
                _bwd_stats[dx.data_ptr()] = (dx, bst, nb.value, N * D * H * W, C)
                return (ncdhw(dx),) + (None,) * ctx.n_extra
        if gskip is None:
            call_act('da_maxpool2_bwd', A(g), A(a), O(dx), N, D, H, W, C, stream())
        else:
            call_act('da_maxpool2_bwd_add', A(g), A(a), A(ndhwc(gskip)), O(dx), N, D, H, W, C, stream())
        return (ncdhw(dx),) + (None,) * ctx.n_extra


class UpsampleNearestFn(Function):
    """F.interpolate(x, size=...) with the default 'nearest' mode (voxel_morph.py:72,74,76,80)."""

    @staticmethod
    def forward(ctx, x, size):
        a = ndhwc(x)
        N, D, H, W, C = a.shape
        Do, Ho, Wo = int(size[0]), int(size[1]), int(size[2])
        out = _empty((N, Do, Ho, Wo, C), a, a.dtype)
        call_act('da_upsample_nearest_fwd', A(a), O(out), N, D, H, W, C, Do, Ho, Wo, stream())
        ctx.dims = (N, D, H, W, C, Do, Ho, Wo)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        N, D, H, W, C, Do, Ho, Wo = ctx.dims
        g = ndhwc(gout)
        dx = _empty((N, D, H, W, C), g, g.dtype)
        call_act('da_upsample_nearest_bwd', A(g), O(dx), N, D, H, W, C, Do, Ho, Wo, stream())
        return ncdhw(dx), None


class WarpFn(Function):
    """deform = disp + identity; warped = grid_sample(src, deform, bilinear, zeros, align_corners=True)
    (voxel_morph.py:85-91, lib/utils.py:89-102).  Returns (warped, deform)."""

    @staticmethod
    def forward(ctx, src, disp):
        s = ndhwc(src)
        u = ndhwc(disp)
        N, D, H, W, C = s.shape
        if tuple(u.shape) != (N, D, H, W, 3):
            raise ValueError('displacement field must be N x 3 x D x H x W matching the source volume')
        out = torch.empty_like(s)
        deform = torch.empty_like(u)
        call('da_warp_fwd', ptr(s), ptr(u), ptr(deform), ptr(out), N, D, H, W, C, stream())
        ctx.save_for_backward(s, u)
        return ncdhw(out), ncdhw(deform)

    @staticmethod
    def backward(ctx, g_out, g_deform):
        s, u = ctx.saved_tensors
        N, D, H, W, C = s.shape
        st = stream()
        d_disp = d_src = None
        go = ndhwc(g_out) if g_out is not None else torch.zeros_like(s)
        if ctx.needs_input_grad[1]:
            d_disp = torch.empty_like(u)
        if ctx.needs_input_grad[0] and DETERMINISTIC:
            # parity runs: order-independent fixed-point accumulation instead of float atomics (da_warp_bwd_dsrc_det)
            d_src = torch.empty_like(s)
            wp, wn = _ws(nat.lib().da_warp_bwd_dsrc_det_ws_bytes(N, D, H, W, C), s)
            call('da_warp_bwd_dsrc_det', ptr(go), ptr(u), ptr(d_src), N, D, H, W, C, wp, wn, st)
            if d_disp is not None:
                call('da_warp_bwd', ptr(go), ptr(s), ptr(u), ptr(d_disp), None, N, D, H, W, C, st)
        else:
            if ctx.needs_input_grad[0]:
                d_src = torch.zeros_like(s)
            call('da_warp_bwd', ptr(go), ptr(s), ptr(u), ptr(d_disp), ptr(d_src), N, D, H, W, C, st)
        if d_disp is not None and g_deform is not None:
            d_disp = d_disp + ndhwc(g_deform)
        return (ncdhw(d_src) if d_src is not None else None), (ncdhw(d_disp) if d_disp is not None else None)


# ------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------
_WEIGHT_TYPES = {'Uniform': 0, 'Simple': 1, 'Volume': 2}


class WarpLabelsFn(Function):
    """warp(one_hot(labels), identity + disp) without the one-hot tensor (joint step, registration phase): N x C x D x H x W."""

    @staticmethod
    def forward(ctx, labels, disp, n_classes):
        u = ndhwc(disp)
        N, D, H, W, _ = u.shape
        lab, nbytes = _labels(labels.reshape(N, -1))
        if lab.shape[1] != D * H * W:
            raise ValueError('label map and displacement field must cover the same volume')
        out = _empty((N, D, H, W, int(n_classes)), u)
        call('da_warp_labels_fwd', ptr(lab), nbytes, ptr(u), ptr(out), N, D, H, W, int(n_classes), stream())
        ctx.cfg = (N, D, H, W, int(n_classes), nbytes)
        ctx.save_for_backward(lab, u)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        lab, u = ctx.saved_tensors
        N, D, H, W, C, nbytes = ctx.cfg
        d_disp = torch.empty_like(u)
        call('da_warp_labels_bwd', ptr(ndhwc(gout)), ptr(lab), nbytes, ptr(u), ptr(d_disp), N, D, H, W, C, stream())
        return None, ncdhw(d_disp), None


# ------------------------------------------------------------------------------------------------
# fused segmentation head + softmax + Dice
# ------------------------------------------------------------------------------------------------
# models/segmentation.py:141-157 calls `output = self.model(images); loss = self.criterion(output, truths)`.  With `model.lazy_head`
# set (SegmentationExperiment and bench.py do, for the softmax-Dice criterion) the network's 1x1x1 output convolution is not run on
# its own: forward() returns a LazyLogits, and DiceLossMultiClass evaluates head + softmax + Dice in one kernel pair (da_head_dice_*)
# that never writes the 629 MB-per-volume logits.  Anything else that touches the object gets real logits via .materialize().
FUSE_HEAD_DICE = True


def head_dice_supported(cin, n_classes):
    return cin in (16, 64) and n_classes in (16, 32)


class LazyLogits(object):
    """The segmentation head's output before anyone has asked for it: (input tensor or LazyAct, weight, bias)."""
    __slots__ = ('x', 'weight', 'bias', '_logits')

    def __init__(self, x, weight, bias):
        self.x, self.weight, self.bias, self._logits = x, weight, bias, None

    @property
    def shape(self):
        xs = self.x.shape
        return torch.Size((xs[0], self.weight.shape[0]) + tuple(xs[2:]))

    def materialize(self):
        if self._logits is None:
            if isinstance(self.x, LazyAct):
                self._logits = Conv1x1Fn.apply(self.x.raw, self.weight, self.bias, (self.x.scale, self.x.shift, self.x.slope))
            else:
                self._logits = Conv1x1Fn.apply(self.x, self.weight, self.bias)
        return self._logits

    def detach(self):
        return self.materialize().detach()


def materialize_logits(x):
    return x.materialize() if isinstance(x, LazyLogits) else x


class HeadDiceFn(Function):
    """Dice(softmax(conv1x1(x)), labels) as one node (da_head_dice_fwd / _bwd): the logits are never written; the backward pass
    recomputes them from x and produces dx, dW, db directly."""

    @staticmethod
    def forward(ctx, x, weight, bias, labels, weight_type, no_bg, eps, *extra):
        pro = extra[0] if extra else None            # (scale, shift, slope) still to be applied to x (LazyAct input)
        ctx.n_extra = len(extra)
        a = ndhwc(x)
        N, D, H, W, Cin = a.shape
        C = weight.shape[0]
        V = D * H * W
        st = stream()
        lab, lb = _labels(labels.reshape(N, -1))
        if lab.shape[1] != V:
            raise ValueError('label map and input must cover the same volume')
        w_io = weight_tio(weight, 'oik').view(Cin, C)
        b = bias.detach().contiguous() if bias is not None else None
        loss = _empty((1,), a)
        coef = _empty((2, N, C), a)
        wsb = nat.lib().da_head_dice_ws_bytes(N, V, Cin, C)
        wp, wn = _ws(wsb, a)
        ps, pt, sl = _pro_args(pro)
        call_act('da_head_dice_fwd', A(a), ps, pt, sl, ptr(w_io), ptr(b), ptr(lab), lb, N, V, Cin, C, _WEIGHT_TYPES[weight_type], 1 if no_bg else 0,
                 float(eps), ptr(loss), ptr(coef), wp, wn, st)
        ctx.wparam = weight
        ctx.cfg = (N, V, Cin, C, lb, wsb, pro[2] if pro is not None else -1.0, bias is not None)
        ctx.save_for_backward(a, w_io, b, lab, coef, pro[0] if pro is not None else None, pro[1] if pro is not None else None)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        a, w_io, b, lab, coef, ps, pt = ctx.saved_tensors
        N, V, Cin, C, lb, wsb, sl, has_bias = ctx.cfg
        st = stream()
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        dx = torch.empty_like(a)
        dw_io = torch.empty_like(w_io)
        db = _empty((C,), a) if has_bias else None
        wp, wn = _ws(wsb, a)
        if (FUSE_BN_BWD_STATS and ps is not None and Cin == 16 and a.dtype == torch.float32 and ps.data_ptr() - 8 * Cin == pt.data_ptr() - 12 * Cin
                and ps.untyped_storage().data_ptr() <= ps.data_ptr() - 8 * Cin):
            # x is the raw output of a conv + BatchNorm block whose statistics are the rows (mean, rstd, scale, shift) of one [4][C] buffer
            # (_bn_forward): that block's BatchNorm-backward sums are accumulated here, where x and its gradient are in registers anyway
            bst = torch.empty((1024, 2, Cin), dtype=torch.float64, device=a.device)
            nb = ctypes.c_int(0)
            call('da_head_dice_bwd_bst', ptr(a), ptr(ps), ptr(pt), float(sl), ctypes.c_void_p(ps.data_ptr() - 8 * Cin), ptr(w_io), ptr(b), ptr(lab), lb,
                 ptr(coef), ptr(gl), ptr(dx), ptr(dw_io), ptr(db), N, V, Cin, C, ptr(bst), 1024, ctypes.byref(nb), wp, wn, st)
            if nb.value > 0:
                _bwd_stats[dx.data_ptr()] = (dx, bst, nb.value, N * V, Cin)
        else:
            call_act('da_head_dice_bwd', A(a), ptr(ps), ptr(pt), float(sl), ptr(w_io), ptr(b), ptr(lab), lb, ptr(coef), ptr(gl),
                     O(dx), ptr(dw_io), ptr(db), N, V, Cin, C, wp, wn, st)
        dw = grad_for_autograd(dw_io.view(1, Cin, C), 'oik', ctx.wparam)
        return (ncdhw(dx), dw, db, None, None, None, None) + (None,) * ctx.n_extra


def fused_anatomy_supported(n_classes):
    """The fused anatomy-loss kernels take class counts whose 4-channel lane groups are a power of two (4, 8, 16, 32, 64)."""
    q = n_classes // 4
    return n_classes % 4 == 0 and 1 <= q <= 16 and (q & (q - 1)) == 0


class LabelWarpDiceFn(Function):
    """Dice(warp(one_hot(labels_m), identity + disp), one_hot(labels_t)) -- the registration phase's anatomy loss (models/joint.py) --
    straight from the two label maps: neither the warped one-hot tensor nor Dice's gradient tensor is materialised
    (da_label_warp_dice_fwd / _bwd).  Same value and d loss / d disp as WarpLabelsFn followed by DiceFn(softmax=False)."""

    @staticmethod
    def forward(ctx, labels_m, labels_t, disp, n_classes, weight_type, no_bg, eps):
        u = ndhwc(disp)
        N, D, H, W, _ = u.shape
        lm, bm = _labels(labels_m.reshape(N, -1))
        lt, bt = _labels(labels_t.reshape(N, -1))
        if lm.shape[1] != D * H * W or lt.shape[1] != D * H * W:
            raise ValueError('label maps and displacement field must cover the same volume')
        C = int(n_classes)
        loss = _empty((1,), u)
        coef = _empty((2, N, C), u)
        wp, wn = _ws(nat.lib().da_label_warp_dice_ws_bytes(N, C), u)
        call('da_label_warp_dice_fwd', ptr(lm), bm, ptr(lt), bt, ptr(u), N, D, H, W, C, _WEIGHT_TYPES[weight_type], 1 if no_bg else 0,
             float(eps), ptr(loss), ptr(coef), wp, wn, stream())
        ctx.cfg = (N, D, H, W, C, bm, bt)
        ctx.save_for_backward(lm, lt, u, coef)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        lm, lt, u, coef = ctx.saved_tensors
        N, D, H, W, C, bm, bt = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        d_disp = torch.empty_like(u)
        call('da_label_warp_dice_bwd', ptr(lm), bm, ptr(lt), bt, ptr(u), ptr(coef), ptr(gl), ptr(d_disp), N, D, H, W, C, stream())
        return None, None, ncdhw(d_disp), None, None, None, None


def _composed(ctx, fn, leaf):
    """Forward of a fused node whose entry declined the shape: the op-by-op composition `fn(leaf)` recorded on a private graph."""
    with torch.enable_grad():
        leaf = leaf.detach().requires_grad_(True)
        loss = fn(leaf)
    ctx.composed = (leaf, loss)
    return loss.detach()


def _composed_backward(ctx, gloss):
    leaf, loss = ctx.composed
    ctx.composed = None
    return torch.autograd.grad(loss, leaf, gloss.detach().to(loss.dtype))[0]


class LabelWarpSoftDiceFn(Function):
    """Dice(source = warp(one_hot(labels_m), identity + disp), target = prob_t) -- the registration phase's anatomy loss for a pair whose fixed
    image has no manual segmentation (models/joint.py; prob_t = the segmentation net's probabilities, a constant).  The warped one-hot tensor
    and Dice's gradient tensor are never materialised (da_softwarp_dice_fwd role 0 / da_softwarp_dice_bwd_disp); gradient to disp only.  Same
    value and d loss / d disp as WarpLabelsFn followed by DiceFn(soft target), which it runs when the entry declines the class count."""

    @staticmethod
    def forward(ctx, labels_m, disp, prob_t, n_classes, weight_type, no_bg, eps):
        u = ndhwc(disp)
        p = ndhwc(prob_t.detach())
        N, D, H, W, _ = u.shape
        C = int(n_classes)
        lm, bm = _labels(labels_m.reshape(N, -1))
        if lm.shape[1] != D * H * W or tuple(p.shape) != (N, D, H, W, C):
            raise ValueError('label map, probabilities and displacement field must cover the same volume')
        loss = _empty((1,), u)
        coef = _empty((2, N, C), u)
        wp, wn = _ws(nat.lib().da_softwarp_dice_ws_bytes(N, C), u)
        ctx.composed = None
        if not call_supported('da_softwarp_dice_fwd', ptr(lm), bm, ptr(u), ptr(p), 0, N, D, H, W, C, _WEIGHT_TYPES[weight_type], 1 if no_bg else 0,
                              float(eps), ptr(loss), ptr(coef), wp, wn, stream()):
            return _composed(ctx, lambda d: DiceFn.apply(WarpLabelsFn.apply(labels_m, d, C), None, prob_t.detach(), weight_type, no_bg, False, eps), disp)
        ctx.cfg = (N, D, H, W, C, bm)
        ctx.save_for_backward(lm, u, p, coef)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        if ctx.composed is not None:
            return None, _composed_backward(ctx, gloss), None, None, None, None, None
        lm, u, p, coef = ctx.saved_tensors
        N, D, H, W, C, bm = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        d_disp = torch.empty_like(u)
        call('da_softwarp_dice_bwd_disp', ptr(lm), bm, ptr(u), ptr(p), ptr(coef), ptr(gl), ptr(d_disp), N, D, H, W, C, stream())
        return None, ncdhw(d_disp), None, None, None, None, None


class SoftmaxLabelWarpDiceFn(Function):
    """Dice(source = softmax(logits), target = warp(one_hot(labels_m), identity + disp)) with disp a constant -- the segmentation phase's anatomy
    loss for a pair whose fixed image has no manual segmentation: the warped manual label of the moving image is the fixed image's pseudo-label.
    Neither the probabilities nor the warped one-hot tensor are written (da_softwarp_dice_fwd role 1); backward is one dense pass over the logits
    (da_softwarp_dice_bwd_logits), no scatter, no atomics.  Falls back to WarpLabelsFn + DiceFn(softmax=True, soft target)."""

    @staticmethod
    def forward(ctx, logits, labels_m, disp, weight_type, no_bg, eps):
        a = ndhwc(logits)
        u = ndhwc(disp.detach())
        N, D, H, W, C = a.shape
        lm, bm = _labels(labels_m.reshape(N, -1))
        if lm.shape[1] != D * H * W or tuple(u.shape) != (N, D, H, W, 3):
            raise ValueError('label map, logits and displacement field must cover the same volume')
        loss = _empty((1,), a)
        coef = _empty((2, N, C), a)
        wp, wn = _ws(nat.lib().da_softwarp_dice_ws_bytes(N, C), a)
        ctx.composed = None
        if a.dtype != torch.float32 or not call_supported('da_softwarp_dice_fwd', ptr(lm), bm, ptr(u), ptr(a), 1, N, D, H, W, C, _WEIGHT_TYPES[weight_type],
                                                          1 if no_bg else 0, float(eps), ptr(loss), ptr(coef), wp, wn, stream()):
            with torch.no_grad():
                target = WarpLabelsFn.apply(labels_m, disp.detach(), C)
            return _composed(ctx, lambda z: DiceFn.apply(z, None, target, weight_type, no_bg, True, eps), logits)
        ctx.cfg = (N, D, H, W, C, bm)
        ctx.save_for_backward(lm, u, a, coef)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        if ctx.composed is not None:
            return _composed_backward(ctx, gloss), None, None, None, None, None
        lm, u, a, coef = ctx.saved_tensors
        N, D, H, W, C, bm = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        dlogits = torch.empty_like(a)
        call('da_softwarp_dice_bwd_logits', ptr(lm), bm, ptr(u), ptr(a), ptr(coef), ptr(gl), ptr(dlogits), N, D, H, W, C, stream())
        return ncdhw(dlogits), None, None, None, None, None


class SegPhaseLossFn(Function):
    """The segmentation phase's two Dice terms as ONE node (models/joint.py):
        l_sup  = Dice(softmax(logits), labels_m)                                   (None labels_m: 0)
        l_anat = Dice(warp(softmax(logits), identity + disp), one_hot(labels_t))    with disp a constant.
    Forward runs the existing kernels (Dice, softmax, warp, Dice).  Backward: Dice's gradient is rank-structured, so the adjoint
    warp collapses to two scatters of 8 atomics per voxel (da_warp_adjoint_labels) and ONE dense pass forms the gradient with respect
    to the logits through the softmax Jacobian for both terms (da_seg_anat_dlogits) -- instead of Dice backward x 2, a 256-atomics-per-
    voxel scatter, softmax backward and the sum of the two logit gradients."""

    @staticmethod
    def forward(ctx, logits, labels_m, disp, labels_t, weight_type, no_bg, eps):
        a = ndhwc(logits)
        u = ndhwc(disp.detach())
        N, D, H, W, C = a.shape
        V = D * H * W
        st = stream()
        wt, nb = _WEIGHT_TYPES[weight_type], 1 if no_bg else 0
        lt, bt = _labels(labels_t.reshape(N, -1))
        lm = coef_s = None
        bm = 0
        loss_s = torch.zeros((1,), dtype=torch.float32, device=a.device)
        # ONE workspace for both Dice entries (a second, larger _ws request on the same stream would replace -- and free -- the first)
        wp, wn = _ws(max(nat.lib().da_dice_ws_bytes(N, V, C), nat.lib().da_warp_dice_ws_bytes(N, C)), a)
        prob = torch.empty_like(a)
        if labels_m is not None:
            lm, bm = _labels(labels_m.reshape(N, -1))
            coef_s = _empty((2, N, C), a)
            # supervised Dice sums and softmax(logits) from ONE pass over the logits (da_softmax_dice_fwd) ...
            if not call_supported('da_softmax_dice_fwd', ptr(a), ptr(lm), bm, ptr(prob), N, V, C, wt, nb, float(eps),
                                  ptr(loss_s), ptr(coef_s), wp, wn, st):
                call('da_dice_fwd', ptr(a), ptr(lm), bm, None, N, V, C, 1, wt, nb, float(eps), ptr(loss_s), ptr(coef_s), wp, wn, st)
                call('da_softmax_fwd', ptr(a), ptr(prob), N * V, C, st)
        else:
            call('da_softmax_fwd', ptr(a), ptr(prob), N * V, C, st)
        loss_a = _empty((1,), a)
        coef_a = _empty((2, N, C), a)
        # ... and the anatomy Dice of the WARPED probabilities without writing the warped tensor (da_warp_dice_fwd)
        wp2, wn2 = wp, wn
        warped = None
        if not call_supported('da_warp_dice_fwd', ptr(prob), ptr(u), ptr(lt), bt, N, D, H, W, C, wt, nb, float(eps),
                              ptr(loss_a), ptr(coef_a), wp2, wn2, st):
            warped = torch.empty_like(a)
            call('da_warp_fwd', ptr(prob), ptr(u), None, ptr(warped), N, D, H, W, C, st)
            call('da_dice_fwd', ptr(warped), ptr(lt), bt, None, N, V, C, 0, wt, nb, float(eps), ptr(loss_a), ptr(coef_a), wp, wn, st)
        ctx.cfg = (N, D, H, W, C, bm, bt)
        ctx.scratch = warped                       # (separate route: dead after the Dice sums, reused as B in backward)
        ctx.save_for_backward(prob, u, lm, lt, coef_s, coef_a)
        return loss_s.reshape(()), loss_a.reshape(())

    @staticmethod
    def backward(ctx, g_s, g_a):
        prob, u, lm, lt, coef_s, coef_a = ctx.saved_tensors
        N, D, H, W, C, bm, bt = ctx.cfg
        st = stream()
        zero = lambda: torch.zeros((1,), dtype=torch.float32, device=prob.device)
        gs = g_s.detach().reshape(1).to(torch.float32).contiguous() if g_s is not None else zero()
        ga = g_a.detach().reshape(1).to(torch.float32).contiguous() if g_a is not None else zero()
        B = ctx.scratch if ctx.scratch is not None else torch.empty_like(prob)
        ctx.scratch = None
        # labels outside [0, C) (the reference's one-hot scatter would raise on them) put their weights into a separate array: uint8 labels
        # with C = 256 cannot have any, everything else gets the array
        A = None if (bt == 1 and C >= 256) else _empty((N, D * H * W), prob)
        call('da_warp_adjoint_labels', ptr(lt), bt, ptr(u), ptr(A), ptr(B), N, D, H, W, C, st)
        dlogits = torch.empty_like(prob)          # B is class-major ([N][C][V]): the gradient cannot be formed in place
        call('da_seg_anat_dlogits', ptr(prob), ptr(lm), bm, ptr(A), ptr(B), ptr(dlogits), ptr(coef_s), ptr(coef_a),
             ptr(gs) if coef_s is not None else None, ptr(ga), N, D * H * W, C, st)
        return ncdhw(dlogits), None, None, None, None, None, None


class DiceFn(Function):
    """DiceLossMultiClass.forward (lib/loss.py:410-476) with the softmax and the one-hot fused in."""

    @staticmethod
    def forward(ctx, source, target, soft_target, weight_type, no_bg, softmax, eps):
        s = ndhwc(source)
        N, C = s.shape[0], s.shape[-1]
        V = s.numel() // (N * C)
        st = stream()
        lab = soft = None
        lab_bytes = 0
        if soft_target is not None:
            soft = ndhwc(soft_target)
        else:
            lab, lab_bytes = _labels(target)
        loss = _empty((1,), s)
        coef = _empty((2, N, C), s)
        wp, wn = _ws(nat.lib().da_dice_ws_bytes(N, V, C), s)
        call('da_dice_fwd', ptr(s), ptr(lab), lab_bytes, ptr(soft), N, V, C, 1 if softmax else 0,
             _WEIGHT_TYPES[weight_type], 1 if no_bg else 0, float(eps), ptr(loss), ptr(coef), wp, wn, st)
        ctx.cfg = (N, V, C, 1 if softmax else 0, lab_bytes)
        ctx.save_for_backward(s, lab, soft, coef)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        s, lab, soft, coef = ctx.saved_tensors
        N, V, C, softmax, lab_bytes = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        d_src = torch.empty_like(s)
        call('da_dice_bwd', ptr(s), ptr(lab), lab_bytes, ptr(soft), ptr(coef), ptr(gl), ptr(d_src), N, V, C, softmax, stream())
        return ncdhw(d_src), None, None, None, None, None, None


class SoftmaxFn(Function):
    """F.softmax(x, dim=1) on N x C x D x H x W (lib/loss.py:427; joint step: probabilities to warp)."""

    @staticmethod
    def forward(ctx, x):
        a = ndhwc(x)
        C = a.shape[-1]
        out = torch.empty_like(a)
        call('da_softmax_fwd', ptr(a), ptr(out), a.numel() // C, C, stream())
        ctx.save_for_backward(out)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, gout):
        out, = ctx.saved_tensors
        C = out.shape[-1]
        g = ndhwc(gout)
        dx = torch.empty_like(out)
        call('da_softmax_bwd', ptr(g), ptr(out), ptr(dx), out.numel() // C, C, stream())
        return ncdhw(dx)


class NCCFn(Function):
    """NormalizedCrossCorrelationLoss.forward (lib/loss.py:493-501)."""

    @staticmethod
    def forward(ctx, x, y):
        nat.require_cuda(x, y)
        a = ndhwc(x) if x.dim() == 5 else x.contiguous()
        b = ndhwc(y) if y.dim() == 5 else y.contiguous()
        N = a.shape[0]
        V = a.numel() // N
        loss = _empty((1,), a)
        stats = torch.empty((N, 8), dtype=torch.float64, device=a.device)
        wp, wn = _ws(nat.lib().da_ncc_ws_bytes(N, V), a)
        call('da_ncc_fwd', ptr(a), ptr(b), N, V, ptr(loss), ptr(stats), wp, wn, stream())
        ctx.five = (x.dim() == 5, y.dim() == 5)
        ctx.save_for_backward(a, b, stats)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        a, b, stats = ctx.saved_tensors
        N = a.shape[0]
        V = a.numel() // N
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        dx = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        call('da_ncc_bwd', ptr(a), ptr(b), ptr(stats), ptr(gl), ptr(dx), ptr(dy), N, V, stream())
        if dx is not None and ctx.five[0]:
            dx = ncdhw(dx)
        if dy is not None and ctx.five[1]:
            dy = ncdhw(dy)
        return dx, dy


MI_STATS_FLOATS = 1096          # DA_MI_STATS_FLOATS (include/deepatlas_hip.h): per sample G [32][32], ga [32], gb [32], MI, padding


class MIFn(Function):
    """Negative mutual information of two images (VoxelMorph's global MutualInformation: Gaussian Parzen windows over `bins` centres in
    [vmin, vmax]); N x 1 x D x H x W or flat N x V inputs, as NCCFn.  The V x bins weight matrices exist only inside the kernels (mi.hip)."""

    @staticmethod
    def forward(ctx, x, y, bins=32, sigma_ratio=1.0, vmin=0.0, vmax=1.0):
        nat.require_cuda(x, y)
        if x.shape != y.shape or x.dim() not in (2, 5) or (x.dim() == 5 and x.shape[1] != 1):
            raise ValueError('mutual information expects two N x 1 x D x H x W volumes or two N x V arrays of the same shape, got %s and %s'
                             % (tuple(x.shape), tuple(y.shape)))
        if x.dtype != torch.float32 or y.dtype != torch.float32:
            raise ValueError('mutual information expects float32 inputs')
        a = ndhwc(x) if x.dim() == 5 else x.contiguous()
        b = ndhwc(y) if y.dim() == 5 else y.contiguous()
        N = a.shape[0]
        V = a.numel() // max(N, 1)
        bins, sigma_ratio, vmin, vmax = int(bins), float(sigma_ratio), float(vmin), float(vmax)
        wsb = nat.lib().da_mi_ws_bytes(N, V, bins)
        if wsb == 0:
            raise nat.NativeError('da_mi_fwd: unsupported arguments (N %d, V %d, bins %d; 2 <= bins <= 32)' % (N, V, bins))
        loss = _empty((1,), a)
        stats = torch.empty((N, MI_STATS_FLOATS), dtype=torch.float32, device=a.device)
        wp, wn = _ws(wsb, a)
        call('da_mi_fwd', ptr(a), ptr(b), N, V, bins, vmin, vmax, sigma_ratio, ptr(loss), ptr(stats), wp, wn, stream())
        ctx.cfg = (bins, vmin, vmax, sigma_ratio, x.dim() == 5, y.dim() == 5)
        ctx.save_for_backward(a, b, stats)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        a, b, stats = ctx.saved_tensors
        bins, vmin, vmax, sigma_ratio, five_x, five_y = ctx.cfg
        N = a.shape[0]
        V = a.numel() // N
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        dx = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        dy = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        call('da_mi_bwd', ptr(a), ptr(b), ptr(stats), ptr(gl), ptr(dx), ptr(dy), N, V, bins, vmin, vmax, sigma_ratio, stream())
        if dx is not None and five_x:
            dx = ncdhw(dx)
        if dy is not None and five_y:
            dy = ncdhw(dy)
        return dx, dy, None, None, None, None


class BendingFn(Function):
    """BendingEnergyLoss.forward, norm='L2' (lib/loss.py:687-730)."""

    @staticmethod
    def forward(ctx, disp, spacing, normalize, norm=2):
        u = ndhwc(disp)
        N, D, H, W, C = u.shape
        if C != 3:
            raise ValueError('bending energy expects a N x 3 x D x H x W displacement field')
        sp = (ctypes_float3(spacing))
        loss = _empty((1,), u)
        wp, wn = _ws(nat.lib().da_bending_ws_bytes(N, D, H, W), u)
        call('da_bending_fwd', ptr(u), N, D, H, W, sp, 1 if normalize else 0, int(norm), ptr(loss), wp, wn, stream())
        ctx.cfg = (tuple(float(s) for s in spacing), bool(normalize), int(norm))
        ctx.save_for_backward(u)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        u, = ctx.saved_tensors
        N, D, H, W, _ = u.shape
        spacing, normalize, norm = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        du = torch.empty_like(u)
        call('da_bending_bwd', ptr(u), ptr(gl), ptr(du), N, D, H, W, ctypes_float3(spacing), 1 if normalize else 0, norm, stream())
        return ncdhw(du), None, None, None


JACOBIAN_PENALTY_POWERS = (1, 2)


def _jacobian_penalty_args(disp, eps, power):
    """Checks of JacobianPenaltyFn that need no device: (eps, power) as (float, int)."""
    if disp.dim() != 5 or disp.shape[1] != 3:
        raise ValueError('the Jacobian penalty expects a N x 3 x D x H x W displacement field, got %s' % (tuple(disp.shape),))
    if disp.dtype != torch.float32:
        raise ValueError('the Jacobian penalty expects a float32 displacement field, got %s' % disp.dtype)
    if isinstance(power, bool) or power not in JACOBIAN_PENALTY_POWERS:
        raise ValueError('the Jacobian penalty takes power 1 or 2, got %r' % (power,))
    if not 0.0 <= float(eps) <= 1.0:
        raise ValueError('the Jacobian penalty takes 0 <= eps <= 1, got %r' % (eps,))
    return float(eps), int(power)


def _jacobian_penalty_fwd(disp, eps, power, want_stats):
    eps, power = _jacobian_penalty_args(disp, eps, power)
    u = ndhwc(disp)
    N, D, H, W, _ = u.shape
    loss = _empty((1,), u)
    det = _empty((N, D, H, W), u)
    stats = torch.empty((2,), dtype=torch.float64, device=u.device) if want_stats else None
    with torch.cuda.device(u.device):
        wp, wn = _ws(nat.lib().da_jacdet_penalty_ws_bytes(N, D, H, W), u)
        call('da_jacdet_penalty_fwd', ptr(u), N, D, H, W, eps, power, ptr(loss), ptr(stats), ptr(det), wp, wn, stream())
    return u, loss, det, stats, eps, power


class JacobianPenaltyFn(Function):
    """Folding penalty mean(max(0, eps - det J)^power) of a displacement field N x 3 x D x H x W (normalised units, as WarpFn takes it), det J
    exactly as jacobian_det computes it (csrc/jacpen.hip).  power 1 or 2, 0 <= eps <= 1; a float32 scalar."""

    @staticmethod
    def forward(ctx, disp, eps=0.0, power=1):
        u, loss, det, _, eps, power = _jacobian_penalty_fwd(disp, eps, power, False)
        ctx.cfg = (eps, power)
        ctx.save_for_backward(u, det)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        u, det = ctx.saved_tensors
        N, D, H, W, _ = u.shape
        eps, power = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        du = torch.empty_like(u)
        with torch.cuda.device(u.device):
            call('da_jacdet_penalty_bwd', ptr(u), ptr(det), ptr(gl), ptr(du), N, D, H, W, eps, power, stream())
        return ncdhw(du), None, None


def jacobian_penalty_stats(disp, eps=0.0, power=1):
    """What the penalty sees of a field, without autograd: (loss float32 scalar, stats float64 [2] = (sum of the penalties over all N V voxels,
    number of active voxels: det J < eps)), both on the device."""
    _, loss, _, stats, _, _ = _jacobian_penalty_fwd(disp.detach(), eps, power, True)
    return loss.reshape(()), stats


INVCONS_STATS = 4          # doubles per sample of da_invcons_fwd's stats: sum |s r|^2, sum |s r|, max |s r|, voxels sampled outside


def _invcons_fwd(u_a, u_b, want_stats, want_resid):
    for name, t in (('u_a', u_a), ('u_b', u_b)):
        if t.dim() != 5 or t.shape[1] != 3:
            raise ValueError('inverse consistency expects N x 3 x D x H x W displacement fields, got %s for %s' % (tuple(t.shape), name))
    if u_a.shape != u_b.shape:
        raise ValueError('inverse consistency expects two fields of one shape, got %s and %s' % (tuple(u_a.shape), tuple(u_b.shape)))
    a, b = ndhwc(u_a), ndhwc(u_b)
    N, D, H, W, _ = a.shape
    loss = _empty((1,), a)
    resid = torch.empty_like(a) if want_resid else None
    stats = torch.empty((N, INVCONS_STATS), dtype=torch.float64, device=a.device) if want_stats else None
    with torch.cuda.device(a.device):
        wp, wn = _ws(nat.lib().da_invcons_ws_bytes(N, D, H, W), a)
        call('da_invcons_fwd', ptr(a), ptr(b), N, D, H, W, ptr(loss), ptr(stats), ptr(resid), wp, wn, stream())
    return a, b, loss, stats, resid


class InverseConsistencyFn(Function):
    """Inverse-consistency penalty of two displacement fields N x 3 x D x H x W (normalised units, as WarpFn takes them), one direction:
    mean over all voxels of |s (u_a(x) + u_b(x + u_a(x)))|^2 in voxels^2, u_b sampled exactly as WarpFn samples (csrc/invcons.hip).
    Gradients reach both fields; the one of u_b is a scatter (float atomics, or the fixed-point accumulation under DETERMINISTIC)."""

    @staticmethod
    def forward(ctx, u_a, u_b):
        a, b, loss, _, resid = _invcons_fwd(u_a, u_b, False, True)
        ctx.save_for_backward(a, b, resid)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        a, b, resid = ctx.saved_tensors
        N, D, H, W, _ = a.shape
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        det = bool(DETERMINISTIC)
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = None
        if ctx.needs_input_grad[1]:
            db = torch.empty_like(b) if det else torch.zeros_like(b)
        with torch.cuda.device(a.device):
            wp, wn = (_ws(nat.lib().da_warp_bwd_dsrc_det_ws_bytes(N, D, H, W, 3), a) if det and db is not None else (None, 0))
            call('da_invcons_bwd', ptr(a), ptr(b), ptr(resid), ptr(gl), ptr(da), ptr(db), N, D, H, W, 1 if det else 0, wp, wn, stream())
        return (ncdhw(da) if da is not None else None), (ncdhw(db) if db is not None else None)


def inverse_consistency_forward(u_a, u_b):
    """Everything da_invcons_fwd writes, without autograd: (loss float32 scalar, stats float64 N x 4 = per sample (sum |s r|^2, sum |s r|,
    max |s r|, voxels sampled outside the volume), the residual r = u_a + u_b(x + u_a) as N x 3 x D x H x W in normalised units), on the device."""
    _, _, loss, stats, resid = _invcons_fwd(u_a.detach(), u_b.detach(), True, True)
    return loss.reshape(()), stats, ncdhw(resid)


def inverse_consistency_stats(u_a, u_b):
    """The composition residual r(x) = u_a(x) + u_b(x + u_a(x)) of two fields in voxels, per sample and without autograd: a dict of float64
    device tensors [N]: mean_vox (mean |s r|), rms_vox, max_vox, outside_frac (share of voxels whose sample point leaves the volume)."""
    a, _, _, stats, _ = _invcons_fwd(u_a.detach(), u_b.detach(), True, False)
    V = float(a.shape[1] * a.shape[2] * a.shape[3])
    return dict(mean_vox=stats[:, 1] / V, rms_vox=(stats[:, 0] / V).sqrt(), max_vox=stats[:, 2].clone(), outside_frac=stats[:, 3] / V)


FIELDINV_STATS = 4         # doubles per sample of da_field_invert / da_field_transport_points: largest final update (voxels), elements not
#                            converged, updates performed, elements whose last sample point leaves the volume


def _fieldinv_args(disp, max_iters, tol_vox, what):
    """Checks of the field-inversion ops that need no device: N x 3 x D x H x W float32, extents >= 2, 1 <= max_iters <= 255, tol_vox >= 0."""
    if not torch.is_tensor(disp) or disp.dim() != 5 or disp.shape[1] != 3:
        raise ValueError('%s expects a N x 3 x D x H x W displacement field, got %s' % (what, tuple(disp.shape) if torch.is_tensor(disp) else type(disp)))
    if disp.dtype != torch.float32:
        raise ValueError('%s expects a float32 displacement field, got %s' % (what, disp.dtype))
    if disp.shape[0] < 1 or min(int(s) for s in disp.shape[2:]) < 2:
        raise ValueError('%s needs at least one sample and >= 2 voxels per axis (align_corners=True), got %s' % (what, tuple(disp.shape)))
    if int(max_iters) != max_iters or not 1 <= int(max_iters) <= 255:
        raise ValueError('%s takes 1 <= max_iters <= 255 (the iteration count is stored in a byte), got %r' % (what, max_iters))
    if not float(tol_vox) >= 0.0:
        raise ValueError('%s takes a tol_vox >= 0 voxels, got %r' % (what, tol_vox))
    return int(max_iters), float(tol_vox)


def invert_field(disp, max_iters=32, tol_vox=1e-3, return_stats=False, return_iters=False):
    """The inverse of the deformation x -> x + u(x): v with (id + u)(id + v) = id, N x 3 x D x H x W float32 in WarpFn's normalised units, by
    the fixed-point iteration v_0 = 0, v_{k+1}(x) = -u(x + v_k(x)) with u sampled trilinearly under border padding (csrc/fieldinv.hip: every
    update of a voxel in registers, one launch).  A voxel stops after the first update of at most tol_vox voxels or after max_iters updates;
    the iteration contracts where u changes by less than one voxel per voxel.  A net's field maps the fixed frame into the moving frame;
    its inverse carries fixed-frame data into the moving frame: warp_labels_nearest(seg_t, invert_field(u)).  No autograd.
    return_stats: also a float64 N x FIELDINV_STATS device tensor per sample (largest final update in voxels, voxels not converged, updates
    performed, voxels whose last sample point left the volume, where the inverse is an extrapolation).  return_iters: also the updates
    performed per voxel, uint8 N x D x H x W.  Returns the field, or a tuple (field[, stats][, iters])."""
    max_iters, tol_vox = _fieldinv_args(disp, max_iters, tol_vox, 'invert_field')
    nat.require_cuda(disp)
    u = ndhwc(disp.detach())
    N, D, H, W, _ = u.shape
    out = torch.empty_like(u)
    stats = torch.empty((N, FIELDINV_STATS), dtype=torch.float64, device=u.device) if return_stats else None
    iters = torch.empty((N, D, H, W), dtype=torch.uint8, device=u.device) if return_iters else None
    with torch.cuda.device(u.device):
        wp, wn = _ws(nat.lib().da_field_invert_ws_bytes(N, D, H, W), u) if return_stats else (None, 0)
        call('da_field_invert', ptr(u), ptr(out), ptr(iters), N, D, H, W, max_iters, tol_vox, ptr(stats), wp, wn, stream())
    res = (ncdhw(out),) + ((stats,) if return_stats else ()) + ((iters,) if return_iters else ())
    return res[0] if len(res) == 1 else res


def transport_points(disp, points, inverse=False, max_iters=32, tol_vox=1e-3, return_stats=False):
    """Points carried through the deformation x -> x + u(x) of `disp` (N x 3 x D x H x W float32, normalised units).  points: N x P x 3 float32
    in voxel index coordinates (x, y, z) = (W, H, D) axis.  inverse False: fixed frame -> moving frame, q = p + s u(p), u sampled trilinearly
    under border padding, s = (size - 1) / 2.  inverse True: moving frame -> fixed frame, the solution x of x + s u(x) = q by the iteration of
    invert_field (same stopping rule, same device function: at the grid nodes it is invert_field's result).  A point outside the volume
    samples the nearest face; a non-finite point gives a NaN row.  No autograd.  Returns N x P x 3, with return_stats also the float64
    N x FIELDINV_STATS statistics of invert_field over each sample's points."""
    max_iters, tol_vox = _fieldinv_args(disp, max_iters, tol_vox, 'transport_points')
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] != 3 or points.shape[0] != disp.shape[0] or points.shape[1] < 1:
        raise ValueError('transport_points expects N x P x 3 points (P >= 1) matching the batch of %d, got %s'
                         % (disp.shape[0], tuple(points.shape) if torch.is_tensor(points) else type(points)))
    if points.dtype != torch.float32:
        raise ValueError('transport_points expects float32 points, got %s' % points.dtype)
    nat.require_cuda(disp, points)
    u = ndhwc(disp.detach())
    p = points.detach().contiguous()
    N, D, H, W, _ = u.shape
    P = int(p.shape[1])
    out = torch.empty_like(p)
    stats = torch.empty((N, FIELDINV_STATS), dtype=torch.float64, device=u.device) if return_stats else None
    with torch.cuda.device(u.device):
        wp, wn = _ws(nat.lib().da_field_points_ws_bytes(N, P), u) if return_stats else (None, 0)
        call('da_field_transport_points', ptr(u), ptr(p), ptr(out), N, D, H, W, P, 1 if inverse else 0, max_iters, tol_vox, ptr(stats), wp, wn, stream())
    return (out, stats) if return_stats else out


def _affine_theta(theta, n):
    """Checks of the affine ops on `theta` that need no device: N x 3 x 4 float32; returns it dense."""
    if theta.dim() != 3 or tuple(theta.shape) != (n, 3, 4):
        raise ValueError('theta must be N x 3 x 4 matching the batch of %d, got %s' % (n, tuple(theta.shape)))
    if theta.dtype != torch.float32:
        raise ValueError('the affine warp expects a float32 theta, got %s' % theta.dtype)
    return theta.contiguous()


def _affine_extents(size):
    if len(size) != 3 or min(int(s) for s in size) < 2:
        raise ValueError('the affine warp needs a volume of >= 2 voxels per axis (align_corners=True), got %s' % (tuple(size),))


class AffineWarpFn(Function):
    """warped = grid_sample(src, affine_grid(theta, src.shape, align_corners=True), bilinear, zeros, align_corners=True) without the grid
    (csrc/affine.hip).  src N x C x D x H x W float32, theta N x 3 x 4 float32 in affine_grid's normalised (x, y, z) convention, the frame of
    WarpFn's deform.  The gradient reaches theta only (one fused pass, deterministic); asking for d src raises NotImplementedError."""

    @staticmethod
    def forward(ctx, src, theta):
        if src.dim() != 5:
            raise ValueError('the affine warp expects a N x C x D x H x W source volume, got %s' % (tuple(src.shape),))
        if src.dtype != torch.float32:
            raise ValueError('the affine warp expects a float32 source volume, got %s' % src.dtype)
        _affine_extents(src.shape[2:])
        th = _affine_theta(theta.detach(), src.shape[0])
        nat.require_cuda(src, th)
        s = ndhwc(src.detach())
        N, D, H, W, C = s.shape
        out = torch.empty_like(s)
        with torch.cuda.device(s.device):
            call('da_affine_warp_fwd', ptr(s), ptr(th), ptr(out), N, D, H, W, C, stream())
        ctx.save_for_backward(s, th)
        return ncdhw(out)

    @staticmethod
    def backward(ctx, g_out):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError('AffineWarpFn has no gradient with respect to the source volume (only theta is optimised)')
        if not ctx.needs_input_grad[1]:
            return None, None
        s, th = ctx.saved_tensors
        N, D, H, W, C = s.shape
        g = ndhwc(g_out)
        d_theta = torch.empty_like(th)
        with torch.cuda.device(s.device):
            wp, wn = _ws(nat.lib().da_affine_warp_ws_bytes(N, D, H, W), s)
            call('da_affine_warp_bwd_theta', ptr(g), ptr(s), ptr(th), ptr(d_theta), N, D, H, W, C, wp, wn, stream())
        return None, d_theta


def affine_disp(theta, disp=None, size=None):
    """The displacement field of an affine map, alone or composed with a field predicted on the pre-aligned image: N x 3 x D x H x W float32
    in WarpFn's normalised units, out(x) = theta (x_n + disp(x), 1) - x_n (da_affine_compose_disp).  WarpFn(src, affine_disp(theta)) samples
    where AffineWarpFn(src, theta) does; WarpFn(src, affine_disp(theta, u)) is WarpFn(AffineWarpFn(src, theta), u) with one interpolation.
    disp None: the affine's own field on a volume of `size` = (D, H, W).  No autograd."""
    if disp is None:
        if size is None:
            raise ValueError('affine_disp needs `size` = (D, H, W) when no displacement field is given')
        D, H, W = (int(s) for s in size)
        u = None
    else:
        if disp.dim() != 5 or disp.shape[1] != 3 or disp.dtype != torch.float32:
            raise ValueError('displacement field must be N x 3 x D x H x W float32')
        if size is not None and tuple(int(s) for s in size) != tuple(disp.shape[2:]):
            raise ValueError('size %s does not match the displacement field %s' % (tuple(size), tuple(disp.shape)))
        D, H, W = (int(s) for s in disp.shape[2:])
    _affine_extents((D, H, W))
    th = _affine_theta(theta.detach(), theta.shape[0] if disp is None else disp.shape[0])
    nat.require_cuda(th, disp)
    if disp is not None:
        u = ndhwc(disp.detach())
    N = th.shape[0]
    out = torch.empty((N, D, H, W, 3), dtype=torch.float32, device=th.device)
    with torch.cuda.device(th.device):
        call('da_affine_compose_disp', ptr(th), ptr(u), ptr(out), N, D, H, W, stream())
    return ncdhw(out)


# ------------------------------------------------------------------------------------------------
# instance refinement of a displacement field (refine.hip); the loop is lib/refine.py refine_field
# ------------------------------------------------------------------------------------------------
REFINE_STATE_FLOATS = 12        # DA_REFINE_STATE_FLOATS (include/deepatlas_hip.h)
REFINE_MAX_BATCH = 64


def refine_lr3(lr_vox, size):
    """Per-channel (x, y, z) step in WarpFn's normalised units of a step of `lr_vox` voxels on a volume of `size` = (D, H, W):
    lr_vox * 2 / (extent - 1), 0 along an axis of extent 1 (nothing moves there)."""
    D, H, W = (int(s) for s in size)
    return tuple(float(lr_vox) * 2.0 / (e - 1) if e > 1 else 0.0 for e in (W, H, D))


def refine_host_state(lr3, betas, eps, step, grad_scale, lambda_sim, it):
    """The REFINE_STATE_FLOATS scalars da_refine_step reads for Adam step `step` (>= 1) and history slot `it`, as a CPU float32 tensor
    (da_refine_host_state: the bias corrections in double, as da_adam_step forms them).  Needs no device."""
    out = (ctypes.c_float * REFINE_STATE_FLOATS)()
    call('da_refine_host_state', (ctypes.c_float * 3)(*[float(v) for v in lr3]), float(betas[0]), float(betas[1]), float(eps), int(step),
         float(grad_scale), float(lambda_sim), int(it), out)
    return torch.tensor(list(out), dtype=torch.float32)


def refine_args(moving, fixed, disp):
    """Checks of the refinement entry points -> (moving N x D x H x W x 1, fixed likewise, N, D, H, W); disp N x 3 x D x H x W is only checked."""
    if moving.dim() != 5 or moving.shape[1] != 1 or tuple(moving.shape) != tuple(fixed.shape):
        raise ValueError('refinement expects two N x 1 x D x H x W volumes of one shape, got %s and %s' % (tuple(moving.shape), tuple(fixed.shape)))
    N, _, D, H, W = (int(s) for s in moving.shape)
    if disp.dim() != 5 or tuple(disp.shape) != (N, 3, D, H, W):
        raise ValueError('displacement field must be N x 3 x D x H x W matching the volumes, got %s for %s' % (tuple(disp.shape), tuple(moving.shape)))
    if moving.dtype != torch.float32 or fixed.dtype != torch.float32 or disp.dtype != torch.float32:
        raise ValueError('refinement expects float32 volumes and a float32 displacement field')
    if not 1 <= N <= REFINE_MAX_BATCH:
        raise ValueError('refinement takes 1..%d samples per call, got %d' % (REFINE_MAX_BATCH, N))
    nat.require_cuda(moving, fixed, disp)
    return ndhwc(moving.detach()), ndhwc(fixed.detach()), N, D, H, W


def refine_moments(mv, fx, u, stats=None, ws=None):
    """stats N x 8 float64 (NCCFn's layout) of NCC(warp(moving, identity + u), fixed), the warped image never written.  mv, fx, u: dense
    N x D x H x W x C tensors (refine_args / ndhwc).  ws: (pointer, size) of a workspace the caller owns (a captured loop), else the shared one."""
    N, D, H, W = (int(s) for s in u.shape[:4])
    if stats is None:
        stats = torch.empty((N, 8), dtype=torch.float64, device=u.device)
    wp, wn = ws if ws is not None else _ws(nat.lib().da_refine_moments_ws_bytes(N, D, H, W), u)
    call('da_refine_moments', ptr(mv), ptr(fx), ptr(u), N, D, H, W, ptr(stats), wp, wn, stream())
    return stats


def refine_step(mv, fx, u, stats, state, g_extra=None, m=None, v=None, grad_out=None, hist=None, update=False):
    """da_refine_step on dense N x D x H x W x C tensors: grad_out (if given) = lambda_sim d(1 - NCC)/du + g_extra; update: Adam on u, m, v in place."""
    N, D, H, W = (int(s) for s in u.shape[:4])
    call('da_refine_step', ptr(mv), ptr(fx), ptr(u), ptr(g_extra), ptr(stats), ptr(state), ptr(m), ptr(v), ptr(grad_out), ptr(hist),
         int(hist.numel()) if hist is not None else 0, N, D, H, W, 1 if update else 0, stream())


def refine_ncc_grad(moving, fixed, disp, lambda_sim=1.0):
    """(1 - NCC, gradient) of lambda_sim * NormalizedCrossCorrelationLoss(WarpFn(moving, disp), fixed) with respect to disp, fused: two passes
    over the volume, neither the warped image nor its cotangent written.  moving, fixed N x 1 x D x H x W, disp N x 3 x D x H x W float32 on
    the GPU; returns a 0-d tensor (unweighted) and N x 3 x D x H x W.  No autograd."""
    mv, fx, N, D, H, W = refine_args(moving, fixed, disp)
    u = ndhwc(disp.detach())
    with torch.cuda.device(u.device):
        stats = refine_moments(mv, fx, u)
        state = refine_host_state((0.0, 0.0, 0.0), (0.9, 0.999), 1e-8, 1, 1.0, lambda_sim, 0).to(u.device)
        grad, hist = torch.empty_like(u), torch.empty((1,), dtype=torch.float32, device=u.device)
        refine_step(mv, fx, u, stats, state, grad_out=grad, hist=hist)
    return hist.reshape(()), ncdhw(grad)


class XentFn(Function):
    """Cross-entropy family of the loss registry (lib/loss.py:739-761) on N x C x D x H x W logits: mode 0 nn.CrossEntropyLoss,
    1 FocalLoss.forward (lib/loss.py:181-213), 2 SoftCrossEntropy.forward with a probability target (:115-154)."""

    @staticmethod
    def forward(ctx, logits, labels, soft_target, alpha, mode, softmax, gamma, ignore_index, reduction):
        a = ndhwc(logits) if logits.dim() == 5 else logits.contiguous()
        nat.require_cuda(a)
        C = a.shape[-1]
        M = a.numel() // C
        lab = soft = None
        lab_bytes = 0
        if soft_target is not None:
            soft = ndhwc(soft_target) if soft_target.dim() == 5 else soft_target.contiguous()
        else:
            lab, lab_bytes = _labels(labels.reshape(-1))
            if lab.numel() != M:
                raise ValueError('target has %d elements for %d voxels' % (lab.numel(), M))
            if CHECK_LABELS:
                # torch.nn.CrossEntropyLoss raises on a target outside [0, C) that is not ignore_index; the kernels skip such voxels (zero loss,
                # zero gradient, not counted).  The check costs a device synchronisation, hence the switch (DA_CHECK_LABELS=1).
                bad = (lab != int(ignore_index)) & ((lab < 0) | (lab >= C)) if lab.dtype == torch.int64 else (lab >= C)
                if bool(bad.any()):
                    raise IndexError('Target %d is out of bounds.' % int(lab[bad][0].item()))
        al = alpha.detach().to(a.device, torch.float32).reshape(-1).contiguous() if alpha is not None else None
        loss, denom = _empty((1,), a), _empty((1,), a)
        wp, wn = _ws(nat.lib().da_xent_ws_bytes(), a)
        call('da_xent_fwd', ptr(a), ptr(lab), lab_bytes, ptr(soft), ptr(al), M, C, int(mode), 1 if softmax else 0, float(gamma),
             int(ignore_index), int(reduction), ptr(loss), ptr(denom), wp, wn, stream())
        ctx.cfg = (M, C, int(mode), 1 if softmax else 0, float(gamma), int(ignore_index), lab_bytes, logits.dim() == 5)
        ctx.save_for_backward(a, lab, soft, al, denom)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        a, lab, soft, al, denom = ctx.saved_tensors
        M, C, mode, softmax, gamma, ignore, lab_bytes, five = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        dx = torch.empty_like(a)
        call('da_xent_bwd', ptr(a), ptr(lab), lab_bytes, ptr(soft), ptr(al), ptr(gl), ptr(denom), ptr(dx), M, C, mode, softmax, gamma, ignore, stream())
        return (ncdhw(dx) if five else dx), None, None, None, None, None, None, None, None


class LNCCFn(Function):
    """Local normalised cross-correlation over all-ones k^3 windows (dilation d, stride s): VoxelMorphLNCC.forward
    (lib/loss.py:599-617: k = filter_size, d = s = 1) and one scale of LNCCLoss.forward (:541-584).  Five box sums as three
    separable passes + fused cc reduction; backward through the adjoint box filter."""

    @staticmethod
    def forward(ctx, I, J, filter_size, eps, dilation=1, stride=1):
        if I.shape != J.shape or I.dim() != 5 or I.shape[1] != 1:
            raise ValueError('LNCC expects two N x 1 x D x H x W volumes of the same shape')
        nat.require_cuda(I); nat.require_cuda(J)
        a, b = I.detach().contiguous().float(), J.detach().contiguous().float()
        N, _, D, H, W = a.shape
        F_, d_, s_ = int(filter_size), int(dilation), int(stride)
        span = d_ * (F_ - 1) + 1
        if min(D, H, W) < span:
            raise RuntimeError('LNCC window %d (dilation %d) larger than the volume %s' % (F_, d_, (D, H, W)))
        od = tuple((L - span) // s_ + 1 for L in (D, H, W))
        loss = _empty((1,), a)
        sums = torch.empty((5, N) + od, dtype=torch.float32, device=a.device)
        wsb = nat.lib().da_lncc_ws_bytes(N, D, H, W, F_, d_, s_)
        wp, wn = _ws(wsb, a)
        call('da_lncc_fwd', ptr(a), ptr(b), N, D, H, W, F_, d_, s_, float(eps), ptr(loss), ptr(sums), wp, wn, stream())
        ctx.cfg = (F_, d_, s_, float(eps), wsb)
        ctx.save_for_backward(a, b, sums)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        a, b, sums = ctx.saved_tensors
        F_, d_, s_, eps, wsb = ctx.cfg
        N, _, D, H, W = a.shape
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        dI = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        dJ = torch.empty_like(a) if ctx.needs_input_grad[1] else None
        wp, wn = _ws(wsb, a)
        call('da_lncc_bwd', ptr(a), ptr(b), ptr(sums), ptr(gl), ptr(dI), ptr(dJ), N, D, H, W, F_, d_, s_, eps, wp, wn, stream())
        return dI, dJ, None, None, None, None


class GradLossFn(Function):
    """gradientLoss.forward (lib/loss.py:640-671), norm 'L2' or 'L1', with the reference's sign quirk along H and W."""

    @staticmethod
    def forward(ctx, disp, spacing, normalize, norm):
        u = ndhwc(disp)
        N, D, H, W, C = u.shape
        if C != 3:
            raise ValueError('gradientLoss expects a N x 3 x D x H x W displacement field')
        loss = _empty((1,), u)
        wp, wn = _ws(nat.lib().da_gradloss_ws_bytes(N, D, H, W), u)
        call('da_gradloss_fwd', ptr(u), N, D, H, W, ctypes_float3(spacing), 1 if normalize else 0, int(norm), ptr(loss), wp, wn, stream())
        ctx.cfg = (tuple(float(s) for s in spacing), bool(normalize), int(norm))
        ctx.save_for_backward(u)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        u, = ctx.saved_tensors
        N, D, H, W, _ = u.shape
        spacing, normalize, norm = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        du = torch.empty_like(u)
        call('da_gradloss_bwd', ptr(u), ptr(gl), ptr(du), N, D, H, W, ctypes_float3(spacing), 1 if normalize else 0, norm, stream())
        return ncdhw(du), None, None, None


def ctypes_float3(v):
    arr = (ctypes.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))
    return ctypes.cast(arr, ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------
# non-differentiable utilities
# ------------------------------------------------------------------------------------------------
def one_hot(mask, n_classes):
    """lib/transforms.py:675-689 mask_to_one_hot for a B x 1 x ... index mask -> B x C x ... float (channels-last)."""
    nat.require_cuda(mask)
    if mask.shape[1] != 1:
        raise ValueError('mask must be B x 1 x ...')
    lab, nbytes = _labels(mask.reshape(mask.shape[0], -1))
    M = lab.numel()
    out = torch.empty((M, n_classes), dtype=torch.float32, device=mask.device)
    call('da_one_hot', ptr(lab), nbytes, ptr(out), M, n_classes, stream())
    spatial = list(mask.shape[2:])
    out = out.reshape([mask.shape[0]] + spatial + [n_classes])
    perm = [0, len(spatial) + 1] + list(range(1, len(spatial) + 1))
    return out.permute(perm)


def identity_grid(size, normalize=True, device='cuda'):
    """lib/utils.py:89-102 get_identity_transform: 3 x D x H x W."""
    D, H, W = int(size[0]), int(size[1]), int(size[2])
    out = torch.empty((3, D, H, W), dtype=torch.float32, device=device)
    call('da_identity_grid', ptr(out), D, H, W, 1 if normalize else 0, stream())
    return out


def argmax_dice_counts(logits, truth):
    """Eval path (models/segmentation.py:188-194): first-max argmax + exact integer overlap counts.
    Returns (counts[N][C][3] int64 = (|pred==c|, |truth==c|, |both|), pred uint8 N x D x H x W)."""
    a = ndhwc(logits)
    N, C = a.shape[0], a.shape[-1]
    V = a.numel() // (N * C)
    lab, nbytes = _labels(truth.reshape(N, -1))
    counts = torch.zeros((N, C, 3), dtype=torch.int64, device=a.device)
    pred = torch.empty((N, V), dtype=torch.uint8, device=a.device)
    call('da_argmax_dice_counts', ptr(a), ptr(lab), nbytes, N, V, C, ptr(counts), ptr(pred), stream())
    return counts, pred.reshape((N,) + tuple(a.shape[1:4]))


def label_overlap_counts(pred, truth, n_class):
    """integer overlap counts of two label maps (any shape with a leading batch axis).
    Returns counts[N][n_class][3] int64 = (|pred==c|, |truth==c|, |both|); labels outside [0, n_class) are ignored."""
    N = pred.shape[0]
    pl, pb = _labels(pred.reshape(N, -1))
    tl, tb = _labels(truth.reshape(N, -1))
    if pl.shape != tl.shape:
        raise ValueError('pred and truth must have the same number of voxels per sample')
    counts = torch.zeros((N, n_class, 3), dtype=torch.int64, device=pl.device)
    call('da_label_overlap_counts', ptr(pl), pb, ptr(tl), tb, N, pl.shape[1], n_class, ptr(counts), stream())
    return counts


AUG_INTERPOLATORS = {'linear': 0, 'nearest': 1}
_LABEL_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}


def _require_label_tensor(t, what):
    """The dtype check of the volume utilities' label maps (the 1 / 4 / 8-byte loader of csrc/common.h), before anything touches the device."""
    if not torch.is_tensor(t) or t.dtype not in _LABEL_BYTES:
        raise ValueError('%s must be a uint8, int32 or int64 tensor, got %s' % (what, getattr(t, 'dtype', type(t)),))


def spatial_resample(image, labels, affine, coef=None, order=0, interpolator='linear'):
    """The resample behind lib/transforms.py's random rigid / B-spline transforms (:161-290), one da_spatial_resample launch per batch.
    image: N x C x D x H x W float32 or None; labels: N x D x H x W uint8 / int32 / int64 or None (not both None); both on the GPU.
    affine: N x 3 x 4 host array, the index-space map q = A[:, :3] i + A[:, 3] with i = (x, y, z) = (w, h, d).  coef: None (order 0) or
    an N x 3 x gz x gy x gx host array of (x, y, z) displacements in INDEX units on the control grid of a B-spline of `order` 1..3,
    added to q.  Image `interpolator` 'linear' or 'nearest', labels nearest; outside the volume 0.1 / 0.
    Returns (image_out, labels_out): fresh tensors, None where the input is None."""
    import numpy as np
    if interpolator not in AUG_INTERPOLATORS:
        raise NotImplementedError("interpolator %r: the device resample implements 'linear' and 'nearest'" % (interpolator,))
    ref = image if image is not None else labels
    if ref is None:
        raise ValueError('spatial_resample needs an image or labels')
    nat.require_cuda(image, labels)
    N = ref.shape[0]
    D, H, W = (int(s) for s in ref.shape[-3:])
    if image is not None:
        if image.dim() != 5 or image.dtype != torch.float32:
            raise ValueError('image must be N x C x D x H x W float32')
        image = image.contiguous()
    if labels is not None:
        if labels.dtype not in _LABEL_BYTES:
            raise ValueError('labels must be uint8, int32 or int64')
        if tuple(labels.shape) != (N, D, H, W):
            raise ValueError('labels must be N x D x H x W matching the image')
        labels = labels.contiguous()
    A = np.asarray(affine, dtype=np.float64).reshape(N, 3, 4)
    # the kernel applies the matrix about o = (W/2, H/2, D/2): q = M (i - o) + (M o + b), which keeps the fp32 terms small
    o = np.array([W // 2, H // 2, D // 2], dtype=np.float64)
    kern = np.concatenate([A[:, :, :3], (A[:, :, :3] @ o + A[:, :, 3])[:, :, None]], axis=2)
    dev = ref.device
    aff = torch.from_numpy(np.ascontiguousarray(kern, dtype=np.float32)).to(dev)
    if order:
        cf = np.ascontiguousarray(coef, dtype=np.float32)
        if cf.ndim != 5 or cf.shape[:2] != (N, 3):
            raise ValueError('coef must be N x 3 x gz x gy x gx')
        gz, gy, gx = cf.shape[2:]
        cft = torch.from_numpy(cf).to(dev)
    else:
        gz = gy = gx = 0
        cft = None
    img_out = torch.empty_like(image) if image is not None else None
    lab_out = torch.empty_like(labels) if labels is not None else None
    with torch.cuda.device(dev):
        call('da_spatial_resample', ptr(image), ptr(img_out), int(image.shape[1]) if image is not None else 0, AUG_INTERPOLATORS[interpolator],
             ptr(labels), ptr(lab_out), _LABEL_BYTES[labels.dtype] if labels is not None else 1,
             ptr(aff), ptr(cft), int(order), int(gx), int(gy), int(gz), N, D, H, W, stream())
    return img_out, lab_out


# ------------------------------------------------------------------------------------------------
# intensity augmentation (csrc/intensity.hip): Gaussian blur, bilateral filter, fused pointwise pass.  No autograd: these run on inputs.
# ------------------------------------------------------------------------------------------------
BLUR_MAX_RADIUS = 16                # DA_BLUR_MAX_RADIUS (include/deepatlas_hip.h)
BLUR_BLOCK = 256                    # voxels one workgroup of a blur line pass takes per loop trip (consecutive along W)
BILATERAL_TILE = (8, 8, 32)         # (td, th, tw) = DA_BILATERAL_TILE_D / _H / _W: the output tile one workgroup filters from LDS
BILATERAL_MAX_RADIUS = 4            # DA_BILATERAL_MAX_RADIUS
BILATERAL_MAX_SAMPLES = 1024        # DA_BILATERAL_MAX_SAMPLES
INTENSITY_FLAGS = {'bias': 1, 'gamma': 2, 'invert': 4, 'linear': 8, 'noise': 16, 'clamp': 32}      # DA_INTENSITY_*
INTENSITY_STREAMS = (2, 3)          # DA_INTENSITY_STREAM_U1 / _U2: the hash streams of the two uniforms
_INTENSITY_PARAM_STRIDE = 8


def _image5(img):
    nat.require_cuda(img)
    if img.dim() not in (4, 5) or img.dtype != torch.float32:
        raise ValueError('image must be C x D x H x W or N x C x D x H x W float32')
    single = img.dim() == 4
    return (img.unsqueeze(0) if single else img).contiguous(), single


_CONST_CACHE = {}


def _const_tensor(arr, device):
    """Device copy of a small read-only host array (taps, tables, flags), kept by content: a transform that repeats its arguments uploads them
    once instead of once per call (a pageable upload makes the host wait for the stream).  The first 64 distinct arrays are kept for the life
    of the process and never released (a kernel on another stream may still be reading one); beyond that an array is uploaded per call."""
    key = (arr.dtype.str, arr.shape, arr.tobytes(), device.type, device.index)
    t = _CONST_CACHE.get(key)
    if t is None:
        t = torch.from_numpy(arr.copy()).to(device)
        if len(_CONST_CACHE) < 64:
            _CONST_CACHE[key] = t
    return t


def _apply_flags(apply, N, device):
    import numpy as np
    flags = np.ones(N, dtype=np.int32) if apply is None else np.asarray(apply).astype(bool).astype(np.int32).reshape(-1)
    if flags.shape[0] != N:
        raise ValueError('apply must hold one flag per sample (%d), got %d' % (N, flags.shape[0]))
    return _const_tensor(flags, device)


def gaussian_blur(img, taps, apply=None):
    """sitk.DiscreteGaussian(img, variance, maximumKernelWidth, maximumError, useImageSpacing=False) (lib/transforms.py:293-306) given its
    taps (lib.transforms.discrete_gaussian_taps): one odd-length vector for all three axes, or three vectors (x, y, z) = (W, H, D) (shorter
    ones are zero-padded to the longest).  Boundary ZeroFluxNeumann (indices clamped).  img C x D x H x W or N x C x D x H x W float32 on
    the GPU; apply: per-sample flags, a sample whose flag is false is copied bit for bit.  Returns a fresh tensor."""
    import numpy as np
    x, single = _image5(img)
    N, C, D, H, W = (int(s) for s in x.shape)
    vecs = [np.asarray(t, dtype=np.float64).reshape(-1) for t in (taps if np.ndim(taps[0]) else [taps] * 3)]
    if len(vecs) != 3 or any(len(v) % 2 == 0 for v in vecs):
        raise ValueError('taps: one odd-length vector, or three (x, y, z)')
    R = max(len(v) for v in vecs) // 2
    tp = np.zeros((3, 2 * R + 1), dtype=np.float32)
    for k, v in enumerate(vecs):
        r = len(v) // 2
        tp[k, R - r:R + r + 1] = v
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    tpt, flags = _const_tensor(tp, x.device), _apply_flags(apply, N, x.device)
    with torch.cuda.device(x.device):
        call('da_gauss_blur3d', ptr(x), ptr(out), ptr(tmp), ptr(tpt), R, ptr(flags), N, C, D, H, W, stream())
    return out[0] if single else out


def bilateral_tables(domain_sigma, range_sigma, n_samples=50, spacing=(1.0, 1.0, 1.0)):
    """Host side of ITK's BilateralImageFilter, fp64: radii (x, y, z) = ceil(2.5 sigma_d / spacing), the domain weights
    [2 rz + 1][2 ry + 1][2 rx + 1] exp(-sum (o_k spacing_k)^2 / (2 sigma_d^2)), the cutoff 4 sigma_r, the table of n_samples entries
    exp(-0.5 (i cutoff / n_samples)^2 / sigma_r^2) and the index scale n_samples / cutoff."""
    import numpy as np
    sp = np.asarray(spacing, dtype=np.float64)
    if not (domain_sigma > 0 and range_sigma > 0 and n_samples >= 1 and (sp > 0).all()):
        raise ValueError('bilateral filter: sigmas, spacing and the number of range samples must be positive')
    r = np.ceil(2.5 * float(domain_sigma) / sp).astype(int)
    ox, oy, oz = (np.arange(-r[k], r[k] + 1) * sp[k] for k in range(3))
    wd = np.exp(-(oz[:, None, None] ** 2 + oy[None, :, None] ** 2 + ox[None, None, :] ** 2) / (2.0 * float(domain_sigma) ** 2))
    cutoff = 4.0 * float(range_sigma)
    table = np.exp(-0.5 * (np.arange(int(n_samples)) * cutoff / int(n_samples)) ** 2 / float(range_sigma) ** 2)
    return tuple(int(v) for v in r), wd, cutoff, table, int(n_samples) / cutoff


def bilateral_filter(img, domain_sigma, range_sigma, n_samples=50, spacing=(1, 1, 1), apply=None):
    """sitk.Bilateral(img, domainSigma, rangeSigma, numberOfRangeGaussianSamples) (lib/transforms.py:308-320) as include/deepatlas_hip.h
    states it; spacing (x, y, z).  Radii beyond BILATERAL_MAX_RADIUS or more than BILATERAL_MAX_SAMPLES range samples raise NativeError
    (DA_ERR_UNSUPPORTED).  Tensors and `apply` as gaussian_blur.  Returns a fresh tensor."""
    import numpy as np
    x, single = _image5(img)
    N, C, D, H, W = (int(s) for s in x.shape)
    (rx, ry, rz), wd, cutoff, table, scale = bilateral_tables(domain_sigma, range_sigma, n_samples, spacing)
    dev = x.device
    wdt = _const_tensor(np.ascontiguousarray(wd, dtype=np.float32), dev)
    tbt = _const_tensor(np.ascontiguousarray(table, dtype=np.float32), dev)
    flags = _apply_flags(apply, N, dev)
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        call('da_bilateral3d', ptr(x), ptr(out), ptr(wdt), ptr(tbt), rx, ry, rz, int(n_samples), float(np.float32(cutoff)), float(np.float32(scale)),
             ptr(flags), N, C, D, H, W, stream())
    return out[0] if single else out


def intensity_params(params, N, seed=0, bias=False):
    """Per-sample parameter dicts -> the N x 8 uint32 table of da_intensity_augment.  A dict may hold 'gamma' (with 'invert'), 'gain' and /
    or 'offset', 'noise_std', 'clamp', 'bias' (default: on when a field is given) and 'seed' (default: `seed`); a stage whose key is
    absent or None is off, and a None entry leaves the whole sample untouched."""
    import numpy as np
    if isinstance(params, dict) or params is None:
        params = [params] * N
    if len(params) != N:
        raise ValueError('params must hold one entry per sample (%d), got %d' % (N, len(params)))
    tab = np.zeros((N, _INTENSITY_PARAM_STRIDE), dtype=np.uint32)
    f32 = tab.view(np.float32)
    for n, p in enumerate(params):
        if p is None:
            continue
        flags = 0
        f32[n, 1], f32[n, 2] = 1.0, 1.0
        if bias and p.get('bias', True):
            flags |= INTENSITY_FLAGS['bias']
        if p.get('gamma') is not None:
            if not p['gamma'] > 0:
                raise ValueError('gamma must be positive')
            flags |= INTENSITY_FLAGS['gamma'] | (INTENSITY_FLAGS['invert'] if p.get('invert') else 0)
            f32[n, 1] = p['gamma']
        if p.get('gain') is not None or p.get('offset') is not None:
            flags |= INTENSITY_FLAGS['linear']
            f32[n, 2] = 1.0 if p.get('gain') is None else p['gain']
            f32[n, 3] = 0.0 if p.get('offset') is None else p['offset']
        if p.get('noise_std') is not None:
            flags |= INTENSITY_FLAGS['noise']
            f32[n, 4] = p['noise_std']
        if p.get('clamp'):
            flags |= INTENSITY_FLAGS['clamp']
        tab[n, 0] = flags
        tab[n, 5] = int(p.get('seed', seed)) & 0xFFFFFFFF
    return tab


def intensity_augment(img, params, bias_coef=None, bias_order=2, seed=0, sample0=0):
    """The fused pointwise intensity pass (one launch, one read and one write of the image): per sample, in this order and each only when
    asked for, bias field x exp(b) (b a scalar B-spline of bias_order 1..3 over bias_coef, a host array N x gz x gy x gx on the control grid
    of lib.transforms.bspline_grid), gamma (optionally inverted), gain / offset, additive Gaussian noise from the counter hash keyed by
    (seed, sample0 + n, element index, stream), clamp to [0, 1].  params: one dict per sample (intensity_params), or one dict for all.
    img C x D x H x W or N x C x D x H x W float32 on the GPU.  Returns a fresh tensor; with every stage off, a bit-exact copy."""
    import numpy as np
    x, single = _image5(img)
    N, C, D, H, W = (int(s) for s in x.shape)
    dev = x.device
    if bias_coef is not None:
        if bias_order not in (1, 2, 3):
            raise ValueError('bias_order %r: orders 1, 2 and 3 are supported' % (bias_order,))
        cf = np.ascontiguousarray(bias_coef, dtype=np.float32)
        if cf.ndim == 3 and single:
            cf = cf[None]
        if cf.ndim != 4 or cf.shape[0] != N:
            raise ValueError('bias_coef must be N x gz x gy x gx')
        gz, gy, gx = (int(s) for s in cf.shape[1:])
        cft, order = torch.from_numpy(cf).to(dev), int(bias_order)
    else:
        gz = gy = gx = order = 0
        cft = None
    tab = torch.from_numpy(intensity_params(params, N, seed, bias=cft is not None).view(np.int32)).to(dev)
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        call('da_intensity_augment', ptr(x), ptr(out), ptr(tab), ptr(cft), order, gx, gy, gz, int(sample0), N, C, D, H, W, stream())
    return out[0] if single else out


# ------------------------------------------------------------------------------------------------
# registration evaluation (csrc/regeval.hip): hard-label warp + overlap counts, Jacobian determinant.  No autograd.
# ------------------------------------------------------------------------------------------------
def _eval_disp(disp):
    u = ndhwc(disp.detach())
    if u.dim() != 5 or u.shape[-1] != 3 or u.dtype != torch.float32:
        raise ValueError('displacement field must be N x 3 x D x H x W float32')
    return u


def _warp_nearest_counts(seg_m, seg_t, disp, n_class, want_counts, want_warped):
    u = _eval_disp(disp)
    N, D, H, W, _ = u.shape
    ml, mb = _labels(seg_m.reshape(seg_m.shape[0], -1))
    if tuple(ml.shape) != (N, D * H * W):
        raise ValueError('label map must be N x D x H x W matching the displacement field')
    tl, tb = None, 1
    counts = warped = None
    if want_counts:
        tl, tb = _labels(seg_t.reshape(seg_t.shape[0], -1))
        if tl.shape != ml.shape:
            raise ValueError('moving and target label maps must have the same shape')
        counts = torch.zeros((N, int(n_class), 3), dtype=torch.int64, device=u.device)
    if want_warped:
        warped = torch.empty((N, D, H, W), dtype=torch.uint8, device=u.device)
    with torch.cuda.device(u.device):
        call('da_warp_labels_nearest_counts', ptr(ml), mb, ptr(tl), tb, ptr(u), N, D, H, W, int(n_class) if want_counts else 0,
             ptr(counts), ptr(warped), stream())
    return counts, warped


def warp_labels_nearest(labels, disp):
    """F.grid_sample(labels, disp + identity, mode='nearest', padding_mode='zeros', align_corners=True) for a label map N x D x H x W
    (uint8 or int64) and a displacement field N x 3 x D x H x W in the layout of WarpFn: the warped map, uint8 N x D x H x W."""
    return _warp_nearest_counts(labels, None, disp, 0, False, True)[1]


def reg_label_counts(seg_m, seg_t, disp, n_class, return_warped=False):
    """Overlap counts of the registration Dice in one pass: counts[N][n_class][3] int64 = (|warp(seg_m)==c|, |seg_t==c|, |both|) with the
    nearest-neighbour warp of warp_labels_nearest; labels outside [0, n_class) are ignored.  Bit-equal to
    label_overlap_counts(warp_labels_nearest(seg_m, disp), seg_t, n_class).  return_warped: (counts, warped uint8 map)."""
    counts, warped = _warp_nearest_counts(seg_m, seg_t, disp, n_class, True, bool(return_warped))
    return (counts, warped) if return_warped else counts


JACOBIAN_STATS = ('sum', 'sumsq', 'min', 'max', 'n_nonpos', 'mean', 'var')


def jacobian_det(disp, return_map=False):
    """Jacobian determinant of x -> x + u(x) for a displacement field N x 3 x D x H x W (normalised units, as WarpFn takes it), u in
    voxels, numpy.gradient differences.  Returns stats, a float64 N x 8 device tensor whose columns are JACOBIAN_STATS (+ one unused);
    return_map: (stats, det N x D x H x W float32)."""
    u = _eval_disp(disp)
    N, D, H, W, _ = u.shape
    stats = torch.empty((N, 8), dtype=torch.float64, device=u.device)
    det = torch.empty((N, D, H, W), dtype=torch.float32, device=u.device) if return_map else None
    with torch.cuda.device(u.device):
        wp, wn = _ws(nat.lib().da_jacobian_det_ws_bytes(N, D, H, W), u)
        call('da_jacobian_det', ptr(u), N, D, H, W, ptr(stats), ptr(det), wp, wn, stream())
    return (stats, det) if return_map else stats


# ------------------------------------------------------------------------------------------------
# multi-atlas label fusion (csrc/regeval.hip): K warped atlas label maps voted per voxel, and the weights of locally weighted voting.
# No autograd.
# ------------------------------------------------------------------------------------------------
FUSION_MAX_ATLASES = 32


def label_fusion(labels, disp, weights=None, return_confidence=False, n_targets=None):
    """Registration-based segmentation of N targets from K atlases each, one da_label_fusion_vote launch: every atlas label map is warped
    to its target grid exactly as warp_labels_nearest warps it, and the warped labels are voted per voxel.
    disp: (N K) x 3 x D x H x W float32, atlas index fastest -- the batch a registration net returns for the N K (atlas, target) pairs.
    labels: K x D x H x W (shared by all targets) or (N K) x D x H x W (per target), uint8 or int64.
    weights: None (majority vote), N x K (per atlas) or N x K x D x H x W (per voxel, e.g. local_msd_weights) float32, >= 0.
    N comes from `weights`, else from K x D x H x W labels (N = batch / K), else from n_targets (default 1: all fields belong to one target).
    score(c) = sum_k w_k [label_k = c] in atlas order; the largest score wins, ties go to the smallest label; confidence = winning score
    / sum_k w_k; a zero total gives label 0 and confidence 0.  Returns the fused map, uint8 N x D x H x W (return_confidence: and the
    confidence, float32 N x D x H x W)."""
    u = _eval_disp(disp)
    NK, D, H, W, _ = u.shape
    if labels.dim() != 4 or tuple(labels.shape[1:]) != (D, H, W):
        raise ValueError('atlas label maps must be K x D x H x W or (N K) x D x H x W matching the displacement fields')
    if labels.dtype not in (torch.uint8, torch.int64):
        raise ValueError('atlas label maps must be uint8 or int64')
    if weights is not None:
        if weights.dtype != torch.float32 or weights.dim() not in (2, 5):
            raise ValueError('weights must be float32, N x K or N x K x D x H x W')
        N, K = int(weights.shape[0]), int(weights.shape[1])
        if weights.dim() == 5 and tuple(weights.shape[2:]) != (D, H, W):
            raise ValueError('per-voxel weights must be N x K x D x H x W matching the displacement fields')
    elif n_targets is not None:
        N = int(n_targets)
        K = NK // N if N > 0 else 0
    elif labels.shape[0] != NK:
        K = int(labels.shape[0])
        N = NK // K if K > 0 else 0
    else:
        N, K = 1, NK
    if N < 1 or K < 1 or N * K != NK:
        raise ValueError('the displacement batch (%d fields) is not N x K = %d x %d' % (NK, N, K))
    if n_targets is not None and int(n_targets) != N:
        raise ValueError('n_targets = %d contradicts the weights (N = %d)' % (int(n_targets), N))
    if labels.shape[0] == K:
        stride = 0
    elif labels.shape[0] == NK:
        stride = K * D * H * W
    else:
        raise ValueError('atlas label maps must be K x D x H x W or (N K) x D x H x W: got %d maps for N = %d, K = %d' % (labels.shape[0], N, K))
    if K > FUSION_MAX_ATLASES:
        raise ValueError('label_fusion takes at most %d atlases per target, got %d' % (FUSION_MAX_ATLASES, K))
    lab, lb = _labels(labels)
    w_atlas = w_voxel = None
    if weights is not None:
        nat.require_cuda(weights)
        if weights.dim() == 2:
            w_atlas = weights.contiguous()
        else:
            w_voxel = weights.contiguous()
    fused = torch.empty((N, D, H, W), dtype=torch.uint8, device=u.device)
    conf = torch.empty((N, D, H, W), dtype=torch.float32, device=u.device) if return_confidence else None
    with torch.cuda.device(u.device):
        call('da_label_fusion_vote', ptr(lab), lb, stride, ptr(u), ptr(w_atlas), ptr(w_voxel), N, K, D, H, W, ptr(fused), ptr(conf), stream())
    return (fused, conf) if return_confidence else fused


def local_msd_weights(warped, target, radius=2, sigma=0.1):
    """Weights of locally weighted voting: w[n][k][x] = exp(-m / (2 sigma^2)), m = the mean over the (2 radius + 1)^3 window around x of
    (warped[n][k] - target[n])^2 (voxels outside the volume contribute 0; the divisor is the full window).
    warped: N x K x D x H x W float32, the atlas images after the trilinear warp (WarpFn) with the fields label_fusion gets;
    target: N x D x H x W or N x 1 x D x H x W float32.  radius 1..4, sigma > 0.  Returns float32 N x K x D x H x W."""
    nat.require_cuda(warped, target)
    if warped.dim() != 5 or warped.dtype != torch.float32:
        raise ValueError('warped atlas images must be N x K x D x H x W float32')
    N, K, D, H, W = (int(s) for s in warped.shape)
    if target.dtype != torch.float32 or tuple(target.shape) not in ((N, D, H, W), (N, 1, D, H, W)):
        raise ValueError('target must be N x D x H x W (or N x 1 x D x H x W) float32 matching the warped atlas images')
    radius = int(radius)
    if not 1 <= radius <= 4:
        raise ValueError('radius must be 1..4, got %r' % (radius,))
    if not float(sigma) > 0.0:
        raise ValueError('sigma must be positive, got %r' % (sigma,))
    beta = 1.0 / (2.0 * float(sigma) * float(sigma))
    a, t = warped.detach().contiguous(), target.detach().contiguous()
    out = torch.empty_like(a)
    with torch.cuda.device(a.device):
        wp, wn = _ws(nat.lib().da_local_msd_weights_ws_bytes(N, K, D, H, W), a)
        call('da_local_msd_weights', ptr(a), ptr(t), N, K, D, H, W, radius, beta, ptr(out), wp, wn, stream())
    return out


# ------------------------------------------------------------------------------------------------
# connected components of a label map, largest-component / minimum-size clean-up (csrc/cc.hip).  No autograd.
# ------------------------------------------------------------------------------------------------
CC_CONNECTIVITIES = (6, 18, 26)
CC_TILE = (4, 8, 32)            # (td, th, tw) = DA_CC_TILE_D / _H / _W (include/deepatlas_hip.h): the tile one workgroup labels in LDS
CC_MAX_CLASSES = 1024           # DA_CC_MAX_CLASSES
CC_STATS = ('n_components', 'largest', 'voxels')      # columns of the [N][n_class][3] statistics


def _cc_args(labels, connectivity, n_class=None, min_size=None):
    """Argument checks of the component ops, all before anything touches the device; returns (N, D, H, W)."""
    _require_label_tensor(labels, 'labels')
    if labels.dim() != 4:
        raise ValueError('labels must be N x D x H x W, got %d dimensions' % labels.dim())
    if connectivity not in CC_CONNECTIVITIES:
        raise ValueError('connectivity must be 6, 18 or 26, got %r' % (connectivity,))
    N, D, H, W = (int(s) for s in labels.shape)
    if N < 1 or D < 1 or H < 1 or W < 1:
        raise ValueError('labels must not be empty, got %s' % (tuple(labels.shape),))
    if D * H * W >= 2 ** 31:
        raise ValueError('a volume of %d x %d x %d has >= 2^31 voxels: raster indices are int32' % (D, H, W))
    if N > 65535:
        raise ValueError('at most 65535 samples per call, got %d' % N)
    if n_class is not None and not 1 <= int(n_class) <= CC_MAX_CLASSES:
        raise ValueError('n_class must be 1..%d, got %r' % (CC_MAX_CLASSES, n_class))
    if min_size is not None and int(min_size) < 1:
        raise ValueError('min_size must be at least 1, got %r' % (min_size,))
    return N, D, H, W


def _cc_label(lab, n_class, connectivity):
    """da_cc_label on a contiguous device label map: (roots, sizes), both int32 N x D x H x W."""
    N, D, H, W = (int(s) for s in lab.shape)
    roots = torch.empty((N, D, H, W), dtype=torch.int32, device=lab.device)
    sizes = torch.empty((N, D, H, W), dtype=torch.int32, device=lab.device)
    wp, wn = _ws(nat.lib().da_cc_ws_bytes(N, D, H, W), lab)
    call('da_cc_label', ptr(lab), _LABEL_BYTES[lab.dtype], N, D, H, W, int(n_class), int(connectivity), ptr(roots), ptr(sizes), wp, wn, stream())
    return roots, sizes


def connected_components(labels, connectivity=6, return_sizes=False, compact=False):
    """Connected components of a label map N x D x H x W (uint8 / int32 / int64; labels <= 0 are background).  Two voxels are connected when
    they hold the same label and are neighbours under `connectivity`: 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners =
    scipy.ndimage.generate_binary_structure(3, 3)).  Samples never interact.
    Returns the root map, int32 N x D x H x W: 0 on background, elsewhere 1 + the smallest raster index (d H + h) W + w of the voxel's
    component -- a function of the input alone, bit-identical from run to run.  compact=True renumbers the components of each sample 1..K in
    the order of their roots, which is the numbering of scipy.ndimage.label when the map holds one label.  return_sizes: (map, sizes), sizes
    int32 N x D x H x W = the component's voxel count at its root's position, 0 elsewhere."""
    N, D, H, W = _cc_args(labels, connectivity)
    nat.require_cuda(labels)
    lab = labels.contiguous()
    with torch.cuda.device(lab.device):
        roots, sizes = _cc_label(lab, 0, connectivity)
        if compact:
            rank = torch.cumsum((sizes.reshape(N, -1) > 0).to(torch.int32), dim=1, dtype=torch.int32)
            flat = roots.reshape(N, -1)
            numbered = rank.gather(1, (flat - 1).clamp_(min=0).long())
            roots = torch.where(flat > 0, numbered, torch.zeros_like(numbered)).reshape(N, D, H, W)
    return (roots, sizes) if return_sizes else roots


def _cc_clean(labels, n_class, connectivity, mode, min_size, return_stats):
    N, D, H, W = _cc_args(labels, connectivity, n_class=n_class, min_size=min_size if mode == 1 else None)
    nat.require_cuda(labels)
    lab = labels.contiguous()
    n_class, V = int(n_class), D * H * W
    out = torch.empty_like(lab)
    stats = best = None
    with torch.cuda.device(lab.device):
        roots, sizes = _cc_label(lab, n_class, connectivity)
        if mode == 0 or return_stats:
            best = torch.zeros((N, n_class), dtype=torch.int64, device=lab.device)
            stats = torch.zeros((N, n_class, 3), dtype=torch.int64, device=lab.device)
            call('da_cc_select', ptr(lab), _LABEL_BYTES[lab.dtype], ptr(sizes), N, V, n_class, ptr(best), ptr(stats), stream())
        call('da_cc_filter', ptr(lab), _LABEL_BYTES[lab.dtype], ptr(roots), ptr(sizes), ptr(best), N, V, n_class, mode,
             int(min_size) if mode == 1 else 1, ptr(out), stream())
    return (out, stats) if return_stats else out


def keep_largest_component(labels, n_class, connectivity=6, return_stats=False):
    """The label map with only the largest connected component of every class 1..n_class-1 in every sample; every other voxel, and every
    label outside [0, n_class), becomes 0.  The largest component is the one with the most voxels, ties go to the component whose first
    voxel in raster order comes first.  Same dtype as the input, which is not modified.
    return_stats: (map, stats), stats int64 N x n_class x 3 with the columns CC_STATS = (number of components, size of the largest, voxels
    of the class) of the INPUT; row 0 (background) is 0."""
    return _cc_clean(labels, n_class, connectivity, 0, None, return_stats)


def remove_small_components(labels, n_class, min_size, connectivity=6, return_stats=False):
    """The label map without the connected components of fewer than `min_size` voxels (and without labels outside [0, n_class)): their
    voxels become 0.  min_size = 1 changes nothing but the out-of-range labels.  return_stats as keep_largest_component."""
    return _cc_clean(labels, n_class, connectivity, 1, min_size, return_stats)


# ------------------------------------------------------------------------------------------------
# exact Euclidean distance transform, signed distance maps of a label map, boundary loss (csrc/edt.hip)
# ------------------------------------------------------------------------------------------------
EDT_LINE_CHUNK = 256            # DA_EDT_LINE_CHUNK (include/deepatlas_hip.h): entries of a line the H and D passes stage in LDS at a time
EDT_MAX_SQ_EXTENT = 2 ** 24     # D^2 + H^2 + W^2 must stay below it: squared distances are exact float32 integers at unit spacing
BOUNDARY_MAX_CLASSES = 64       # channels the boundary-loss kernels keep in registers


def _edt_spacing(spacing):
    try:
        sp = tuple(float(s) for s in spacing)
    except TypeError:
        raise ValueError('spacing must be three positive numbers (sD, sH, sW), got %r' % (spacing,))
    if len(sp) != 3 or not all(0.0 < s < float('inf') for s in sp):
        raise ValueError('spacing must be three positive finite numbers (sD, sH, sW), got %r' % (spacing,))
    return sp


def _edt_extents(t, what):
    """Shape checks of the distance ops, before anything touches the device; returns (N, D, H, W)."""
    if t.dim() != 4:
        raise ValueError('%s must be N x D x H x W, got %d dimensions' % (what, t.dim()))
    N, D, H, W = (int(s) for s in t.shape)
    if N < 1 or D < 1 or H < 1 or W < 1:
        raise ValueError('%s must not be empty, got %s' % (what, tuple(t.shape)))
    if N > 65535:
        raise ValueError('at most 65535 samples per call, got %d' % N)
    if D * D + H * H + W * W >= EDT_MAX_SQ_EXTENT:
        raise ValueError('a volume of %d x %d x %d has D^2 + H^2 + W^2 >= 2^24: squared distances would not be exact in float32' % (D, H, W))
    if D * H * W >= 2 ** 31:
        raise ValueError('a volume of %d x %d x %d has >= 2^31 voxels' % (D, H, W))
    return N, D, H, W


def distance_transform_edt(mask, spacing=(1, 1, 1), squared=False):
    """Exact Euclidean distance transform of N x D x H x W masks (bool, uint8, int32 or int64; nonzero = foreground), scipy's convention:
    0 on the zero voxels, elsewhere the distance to the nearest zero voxel of the same sample, with the voxel spacing (sD, sH, sW) =
    scipy.ndimage.distance_transform_edt(mask[n], sampling=spacing).  squared=True returns the squared distance; with unit spacing it is an
    exact integer.  A sample without a zero voxel returns +inf everywhere (scipy's result is meaningless in that case: it measures to a
    voxel outside the array).  float32, no autograd."""
    if not torch.is_tensor(mask) or (mask.dtype != torch.bool and mask.dtype not in _LABEL_BYTES):
        raise ValueError('mask must be a bool, uint8, int32 or int64 tensor, got %s' % (getattr(mask, 'dtype', type(mask)),))
    N, D, H, W = _edt_extents(mask, 'mask')
    sp = _edt_spacing(spacing)
    nat.require_cuda(mask)
    m = mask.contiguous()
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    out = torch.empty((N, D, H, W), dtype=torch.float32, device=m.device)
    with torch.cuda.device(m.device):
        wp, wn = _ws(nat.lib().da_edt_ws_bytes(N, 1, D, H, W), m)
        call('da_edt_sq', ptr(m), _LABEL_BYTES[m.dtype], N, D, H, W, sp[0], sp[1], sp[2], 0 if squared else 1, ptr(out), wp, wn, stream())
    return out


def _boundary_classes(n_class, classes):
    """The class list of the signed maps / the boundary loss: default 1 .. n_class - 1 (no background); distinct, inside [0, n_class)."""
    n_class = int(n_class)
    if n_class < 1:
        raise ValueError('n_class must be at least 1, got %r' % (n_class,))
    cl = list(range(1, n_class)) if classes is None else [int(c) for c in classes]
    if not cl:
        raise ValueError('the class list is empty (n_class = %d without the background leaves nothing)' % n_class)
    if len(set(cl)) != len(cl) or min(cl) < 0 or max(cl) >= n_class:
        raise ValueError('classes must be distinct and inside [0, %d), got %r' % (n_class, cl))
    return cl


def signed_distance_maps(labels, n_class, classes=None, spacing=(1, 1, 1)):
    """Signed Euclidean distance maps of an index label map N x D x H x W (uint8 / int32 / int64), one per class of `classes` (default
    1 .. n_class - 1: the background is left out): N x K' x D x H x W float32, contiguous (planar, the layout BoundaryLossFn reads).
    Outside class c: + the distance to the nearest voxel of class c; inside: - the distance to the nearest voxel not of class c; a class
    absent from a sample, or filling it, gives 0 everywhere in that sample, so it contributes nothing to the boundary loss (as in Kervadec's
    code).  This is the plain signed distance: Kervadec's one_hot2dist shifts the inside by one voxel, -(d - 1); this does not.
    Labels outside [0, n_class) belong to no class.  The one-hot tensor is never built.  No autograd."""
    _require_label_tensor(labels, 'labels')
    N, D, H, W = _edt_extents(labels, 'labels')
    cl = _boundary_classes(n_class, classes)
    sp = _edt_spacing(spacing)
    nat.require_cuda(labels)
    lab = labels.contiguous()
    cls = torch.tensor(cl, dtype=torch.int32, device=lab.device)
    phi = torch.empty((N, len(cl), D, H, W), dtype=torch.float32, device=lab.device)
    with torch.cuda.device(lab.device):
        wp, wn = _ws(nat.lib().da_edt_ws_bytes(N, len(cl), D, H, W), lab)
        call('da_signed_distance_maps', ptr(lab), _LABEL_BYTES[lab.dtype], ptr(cls), len(cl), N, D, H, W, sp[0], sp[1], sp[2], ptr(phi), wp, wn, stream())
    return phi


class BoundaryLossFn(Function):
    """Boundary loss (Kervadec et al.): mean over samples, chosen classes and voxels of softmax(logits)_c * phi_c.
    logits N x K x D x H x W float32; phi N x K' x D x H x W float32 = signed_distance_maps(...) for `classes` (K' entries, distinct,
    inside [0, K)).  The gradient goes to the logits only."""

    @staticmethod
    def forward(ctx, logits, phi, classes):
        if logits.dim() != 5 or phi.dim() != 5 or logits.dtype != torch.float32 or phi.dtype != torch.float32:
            raise ValueError('logits and phi must be float32 N x K x D x H x W / N x K\' x D x H x W')
        N, K = int(logits.shape[0]), int(logits.shape[1])
        cl = _boundary_classes(K, classes)
        if tuple(phi.shape) != (N, len(cl)) + tuple(logits.shape[2:]):
            raise ValueError('phi is %s for logits %s and %d classes' % (tuple(phi.shape), tuple(logits.shape), len(cl)))
        if K > BOUNDARY_MAX_CLASSES:
            raise ValueError('at most %d channels, got %d' % (BOUNDARY_MAX_CLASSES, K))
        a = ndhwc(logits.detach())
        nat.require_cuda(a, phi)
        p = phi.detach().contiguous()
        V = a.numel() // (N * K)
        slots_host = [-1] * K
        for j, c in enumerate(cl):
            slots_host[c] = j
        slots = torch.tensor(slots_host, dtype=torch.int32, device=a.device)
        loss = _empty((1,), a)
        with torch.cuda.device(a.device):
            wp, wn = _ws(nat.lib().da_boundary_loss_ws_bytes(N), a)
            call('da_boundary_loss_fwd', ptr(a), ptr(p), ptr(slots), N, V, K, len(cl), ptr(loss), wp, wn, stream())
        ctx.cfg = (N, V, K, len(cl))
        ctx.save_for_backward(a, p, slots)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        a, p, slots = ctx.saved_tensors
        N, V, K, Kp = ctx.cfg
        gl = gloss.detach().reshape(1).to(torch.float32).contiguous()
        dx = torch.empty_like(a)
        with torch.cuda.device(a.device):
            call('da_boundary_loss_bwd', ptr(a), ptr(p), ptr(slots), ptr(gl), N, V, K, Kp, ptr(dx), stream())
        return ncdhw(dx), None, None


# ------------------------------------------------------------------------------------------------
# surface-distance metrics of two label maps: Hausdorff, its percentile, ASSD (csrc/edt.hip)
# ------------------------------------------------------------------------------------------------
SURFACE_STATS = ('n_pred', 'n_truth', 'hd', 'hd_pct', 'assd', 'asd_pred_truth', 'asd_truth_pred')
SURFACE_CONNECTIVITIES = (6, 18, 26)      # scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3)
SURFACE_MAX_CLASSES = 65535               # entries of a class list: a grid dimension of the counting pass


def _surface_connectivity(connectivity):
    if connectivity not in SURFACE_CONNECTIVITIES:
        raise ValueError('connectivity must be 6, 18 or 26, got %r' % (connectivity,))
    return int(connectivity)


def _surface_labels(t, what):
    _require_label_tensor(t, what)
    return _edt_extents(t, what)


def label_surface(labels, connectivity=6):
    """Bool mask N x D x H x W: the voxel is a surface voxel of its own label -- it has a neighbour under the connectivity (6, 18 or 26) with
    another label or outside the volume; for every label c the mask restricted to c is A & ~scipy.ndimage.binary_erosion(A, structure) with
    A = (labels == c).  labels: uint8, int32 or int64; the predicate is the one surface_distance_stats measures between."""
    N, D, H, W = _surface_labels(labels, 'labels')
    conn = _surface_connectivity(connectivity)
    nat.require_cuda(labels)
    lab = labels.contiguous()
    out = torch.empty((N, D, H, W), dtype=torch.uint8, device=lab.device)
    with torch.cuda.device(lab.device):
        call('da_label_surface', ptr(lab), _LABEL_BYTES[lab.dtype], N, D, H, W, conn, ptr(out), stream())
    return out.view(torch.bool)


def surface_distance_stats(pred, truth, n_class, classes=None, spacing=(1, 1, 1), connectivity=6, percentile=95.0):
    """Surface-distance metrics of two index label maps N x D x H x W (uint8, int32 or int64, each its own; views are accepted), one row per
    sample and class of `classes` (default 1 .. n_class - 1): float64 N x K' x 7 on the device, columns SURFACE_STATS.
    With d_PT the Euclidean distances, under `spacing` = (sD, sH, sW), of the surface voxels (label_surface) of class c in `pred` to the
    nearest surface voxel of class c in `truth`, and d_TP the other way:  hd = max(max d_PT, max d_TP);  hd_pct = numpy's linear percentile
    of the pooled d_PT and d_TP;  asd_pred_truth = mean d_PT, asd_truth_pred = mean d_TP, assd their mean (medpy's hd, hd95, asd, assd).
    n_pred and n_truth are the surface voxel counts; where a class is absent from either map of a sample the five metrics are NaN.
    Labels outside [0, n_class) belong to no class.  Exact at unit spacing, bit-identical from run to run.  No autograd."""
    N, D, H, W = _surface_labels(pred, 'pred')
    _surface_labels(truth, 'truth')
    if tuple(pred.shape) != tuple(truth.shape):
        raise ValueError('pred is %s and truth is %s: the shapes must agree' % (tuple(pred.shape), tuple(truth.shape)))
    cl = _boundary_classes(n_class, classes)
    if len(cl) > SURFACE_MAX_CLASSES:
        raise ValueError('at most %d classes per call, got %d' % (SURFACE_MAX_CLASSES, len(cl)))
    sp = _edt_spacing(spacing)
    conn = _surface_connectivity(connectivity)
    try:
        pct = float(percentile)
    except (TypeError, ValueError):
        raise ValueError('percentile must be a number in (0, 100], got %r' % (percentile,))
    if not 0.0 < pct <= 100.0:
        raise ValueError('percentile must be in (0, 100], got %r' % (percentile,))
    nat.require_cuda(pred, truth)
    if truth.device != pred.device:
        raise ValueError('pred is on %s and truth on %s' % (pred.device, truth.device))
    p, t = pred.contiguous(), truth.contiguous()
    cls = torch.tensor(cl, dtype=torch.int32, device=p.device)
    out = torch.empty((N, len(cl), len(SURFACE_STATS)), dtype=torch.float64, device=p.device)
    with torch.cuda.device(p.device):
        wp, wn = _ws(nat.lib().da_surface_dist_ws_bytes(N, len(cl), D, H, W), p)
        call('da_surface_dist_stats', ptr(p), _LABEL_BYTES[p.dtype], ptr(t), _LABEL_BYTES[t.dtype], ptr(cls), len(cl), N, D, H, W,
             sp[0], sp[1], sp[2], conn, pct, ptr(out), wp, wn, stream())
    return out


# ------------------------------------------------------------------------------------------------
# volume preprocessing (preprocess.hip; lib/transforms.py:9-68, :269-284, :692-706): resample to a voxel size, moments, percentiles,
# intensity rescale, label look-up.  No autograd.
# ------------------------------------------------------------------------------------------------
PREPROCESS_DTYPE_CODE = {torch.float32: 0, torch.float64: 1, torch.int16: 2, torch.uint8: 3, torch.int32: 4}
RESAMPLE_INTERPOLATORS = {'linear': 0, 'nearest': 1}
PREPROCESS_MAX_VOXELS = 2 ** 31
LABEL_LUT_MAX = 65536


def resample_axis_table(n_in, n_out, scale, offset, interpolator='nearest'):
    """One axis of da_resample_axes, on the host in float64 (pure numpy, no GPU): output index o reads the continuous input index
    q = scale * o + offset (one multiply, one add).  Returns (lower int32[n_out], upper int32[n_out], fraction float32[n_out], inside bool[n_out]).
    Inside iff -0.5 <= q < n_in - 0.5.  'nearest': lower = upper = clamp(floor(q + 0.5), 0, n_in - 1) (ties round up), fraction 0.  'linear':
    f = floor(q), lower = clamp(f, 0, n_in - 1), upper = min(lower + 1, n_in - 1), fraction float32(q - f); for q < 0 lower 0 and fraction 0.
    This is ITK ResampleImageFilter's documented behaviour (the buffer test on the continuous index, edge-clamped taps); agreement with ITK
    itself is not tested.  Entries outside keep their clamped taps here; resample_volume marks them for the kernel."""
    import numpy as np
    if interpolator not in RESAMPLE_INTERPOLATORS:
        raise ValueError("interpolator %r: 'nearest' or 'linear'" % (interpolator,))
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError('resample_axis_table needs n_in >= 1 and n_out >= 1, got %d and %d' % (n_in, n_out))
    scale, offset = float(scale), float(offset)
    if not (np.isfinite(scale) and np.isfinite(offset)):
        raise ValueError('scale and offset must be finite')
    q = np.float64(scale) * np.arange(n_out, dtype=np.float64) + np.float64(offset)
    inside = (q >= -0.5) & (q < n_in - 0.5)
    if interpolator == 'nearest':
        lo = np.clip(np.floor(q + 0.5), 0, n_in - 1).astype(np.int32)
        return lo, lo.copy(), np.zeros(n_out, dtype=np.float32), inside
    f = np.floor(q)
    lo = np.clip(f, 0, n_in - 1).astype(np.int32)
    hi = np.minimum(lo + 1, n_in - 1).astype(np.int32)
    frac = np.where(q < 0, 0.0, q - f).astype(np.float32)
    return lo, hi, frac, inside


def _pack_axis_tables(tables):
    """Three resample_axis_table results (D, H, W) -> the int32 [Do + Ho + Wo][3] array of da_resample_axes (lower tap -1 = outside)."""
    import numpy as np
    rows = []
    for lo, hi, frac, inside in tables:
        t = np.empty((len(lo), 3), dtype=np.int32)
        t[:, 0] = np.where(inside, lo, -1)
        t[:, 1] = hi
        t[:, 2] = np.ascontiguousarray(frac, dtype=np.float32).view(np.int32)
        rows.append(t)
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def _volume4(vol, what='volume'):
    if not torch.is_tensor(vol) or vol.dim() not in (3, 4):
        raise ValueError('%s must be a D x H x W or C x D x H x W tensor' % what)
    if vol.dtype not in PREPROCESS_DTYPE_CODE:
        raise ValueError('%s dtype %s: float32, float64, int16, uint8 or int32' % (what, vol.dtype))
    if vol.numel() == 0:
        raise ValueError('%s is empty' % what)
    if vol.numel() >= PREPROCESS_MAX_VOXELS:
        raise ValueError('%s has %d elements: the preprocessing kernels take fewer than 2^31' % (what, vol.numel()))
    return vol.dim() == 3


def resample_volume(vol, out_size, scale, offset, interpolator='nearest', default=0):
    """Axis-aligned resample of a D x H x W or C x D x H x W device volume onto a grid out_size = (Do, Ho, Wo): output index o of each axis reads
    input index scale * o + offset (scale, offset: three numbers each, (D, H, W) order), by the rule of resample_axis_table.  'nearest' returns
    the source dtype bit for bit, 'linear' float32; voxels outside on any axis get `default`.  A negative scale with offset n - 1 is a flip."""
    single = _volume4(vol)
    if interpolator not in RESAMPLE_INTERPOLATORS:
        raise ValueError("interpolator %r: 'nearest' or 'linear'" % (interpolator,))
    if len(out_size) != 3 or len(scale) != 3 or len(offset) != 3:
        raise ValueError('out_size, scale and offset take three values each (D, H, W)')
    v = vol.unsqueeze(0) if single else vol
    C, D, H, W = (int(s) for s in v.shape)
    Do, Ho, Wo = (int(s) for s in out_size)
    if min(Do, Ho, Wo) < 1:
        raise ValueError('out_size must be positive, got %s' % (tuple(out_size),))
    if C * Do * Ho * Wo >= PREPROCESS_MAX_VOXELS:
        raise ValueError('the output has %d elements: the preprocessing kernels take fewer than 2^31' % (C * Do * Ho * Wo))
    packed = _pack_axis_tables([resample_axis_table(n, m, s, o, interpolator) for n, m, s, o in zip((D, H, W), (Do, Ho, Wo), scale, offset)])
    nat.require_cuda(v)
    v = v.contiguous()
    tab = _const_tensor(packed, v.device)
    out = torch.empty((C, Do, Ho, Wo), dtype=torch.float32 if interpolator == 'linear' else v.dtype, device=v.device)
    with torch.cuda.device(v.device):
        call('da_resample_axes', ptr(v), PREPROCESS_DTYPE_CODE[v.dtype], ptr(out), RESAMPLE_INTERPOLATORS[interpolator], C, D, H, W, Do, Ho, Wo,
             ptr(tab), float(default), stream())
    return out[0] if single else out


def volume_moments(vol):
    """(count of finite voxels, their mean, their unbiased variance) of a device volume as Python floats; two passes in double, fixed order."""
    _volume4(vol)
    nat.require_cuda(vol)
    v = vol.contiguous()
    out = torch.empty(3, dtype=torch.float64, device=v.device)
    with torch.cuda.device(v.device):
        wp, wn = _ws(nat.lib().da_volume_moments_ws_bytes(v.numel()), v)
        call('da_volume_moments', ptr(v), PREPROCESS_DTYPE_CODE[v.dtype], v.numel(), ptr(out), wp, wn, stream())
    c, m, s2 = out.tolist()
    return c, m, s2


def volume_order_statistics(vol, percentiles):
    """The raw result of da_volume_percentiles for one or two percentiles: dict with 'percentiles' (list of doubles), 'order_statistics'
    (per percentile the (lower, upper) float32 order statistics it interpolates), 'count' (non-NaN values) and 'nan_count'."""
    _volume4(vol)
    ps = [float(p) for p in (percentiles if hasattr(percentiles, '__len__') else [percentiles])]
    if not 1 <= len(ps) <= 2:
        raise ValueError('one or two percentiles per call, got %d' % len(ps))
    if any(not 0.0 <= p <= 100.0 for p in ps):
        raise ValueError('percentiles must be in [0, 100], got %r' % (ps,))
    nat.require_cuda(vol)
    v = vol.contiguous()
    out = torch.empty(8, dtype=torch.float64, device=v.device)
    arr = (ctypes.c_double * len(ps))(*ps)
    with torch.cuda.device(v.device):
        wp, wn = _ws(nat.lib().da_volume_percentiles_ws_bytes(v.numel()), v)
        call('da_volume_percentiles', ptr(v), PREPROCESS_DTYPE_CODE[v.dtype], v.numel(), arr, len(ps), ptr(out), wp, wn, stream())
    o = out.tolist()
    return {'percentiles': o[:len(ps)], 'order_statistics': [(o[2 + 2 * j], o[3 + 2 * j]) for j in range(len(ps))],
            'count': int(o[6]), 'nan_count': int(o[7])}


def volume_percentiles(vol, percentiles):
    """numpy.percentile(x, p) (the 'linear' rule) of the float32 values of a device volume, NaNs left out, for one or two p: a tuple of doubles.
    Exact order statistics by a three-digit radix select on the device."""
    return tuple(volume_order_statistics(vol, percentiles)['percentiles'])


def affine_intensity(vol, a, b, clamp=False):
    """(x - a) / b as float32 (a, b rounded to float32), optionally clamped to [0, 1]; b == 0 gives zeros.  Same shape as vol."""
    _volume4(vol)
    nat.require_cuda(vol)
    v = vol.contiguous()
    out = torch.empty(v.shape, dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        call('da_affine_intensity_to_f32', ptr(v), PREPROCESS_DTYPE_CODE[v.dtype], ptr(out), v.numel(), float(a), float(b), 1 if clamp else 0, stream())
    return out


def label_lut(labels, lut):
    """lut[label] for a uint8 / int32 device label volume (same dtype out); lut: at most 65536 integers; labels outside the table map to 0."""
    import numpy as np
    _volume4(labels, 'labels')
    if labels.dtype not in (torch.uint8, torch.int32):
        raise ValueError('labels must be uint8 or int32, got %s' % labels.dtype)
    table = np.ascontiguousarray(np.asarray(lut).reshape(-1), dtype=np.int32)
    if not 1 <= table.shape[0] <= LABEL_LUT_MAX:
        raise ValueError('the look-up table takes 1..%d entries, got %d' % (LABEL_LUT_MAX, table.shape[0]))
    nat.require_cuda(labels)
    v = labels.contiguous()
    out = torch.empty_like(v)
    t = _const_tensor(table, v.device)
    with torch.cuda.device(v.device):
        call('da_label_lut', ptr(v), PREPROCESS_DTYPE_CODE[v.dtype], ptr(out), v.numel(), ptr(t), int(table.shape[0]), stream())
    return out


# ------------------------------------------------------------------------------------------------
# random crops (csrc/crop.hip; lib/transforms.py:322-505)
# ------------------------------------------------------------------------------------------------
CROP_LABEL_DTYPE_CODE = {torch.uint8: 3, torch.int32: 4, torch.int64: 5}
CROP_STREAM = 4                     # DA_CROP_STREAM (csrc/counter_hash.h): the hash stream of the sampler's draws
CROP_MAX_DRAWS = 65536
CROP_MAX_ROW = 32768                # longest row (W) the row pass stages in LDS


def _crop_labels(labels):
    if not torch.is_tensor(labels) or labels.dim() != 4:
        raise ValueError('labels must be an N x D x H x W tensor')
    if labels.dtype not in CROP_LABEL_DTYPE_CODE:
        raise ValueError('labels dtype %s: uint8, int32 or int64' % labels.dtype)
    if labels.numel() == 0:
        raise ValueError('labels is empty')
    nat.require_cuda(labels)
    return labels.contiguous()


def _crop_window(window, extents):
    if len(window) != 3:
        raise ValueError('window takes three values (wd, wh, ww)')
    w = tuple(int(v) for v in window)
    if any(a < 1 or a > s for a, s in zip(w, extents)):
        raise ValueError('window %s must lie in 1..extent of a %s volume' % (w, tuple(extents)))
    return w


def _int3_array(v):
    arr = (ctypes.c_int * 3)(int(v[0]), int(v[1]), int(v[2]))
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def crop_domain(extents, window, include_last=False):
    """Starts per axis of the crop sampler: max(S - w, 1) (what random_3d_coordinates draws: randint's upper end is exclusive, so the last
    start is never used), or S - w + 1 with include_last."""
    return tuple((s - w + 1) if include_last else max(s - w, 1) for s, w in zip(extents, window))


def crop_conditions(classes, min_counts):
    """Host half of sample_crop_starts: the draws' (class, min_count) pairs -> (conds int32 [Q][2] sorted by class then min_count, draw_cond
    int32 [P]: the row of conds of each draw, -1 for class None).  Draws that share a class sit next to each other and share its passes."""
    import numpy as np
    classes, min_counts = list(classes), list(min_counts)
    if len(classes) != len(min_counts) or not 1 <= len(classes) <= CROP_MAX_DRAWS:
        raise ValueError('classes and min_counts take one entry per draw, 1..%d draws' % CROP_MAX_DRAWS)
    pairs = []
    for c, m in zip(classes, min_counts):
        if c is None:
            pairs.append(None)
            continue
        c, m = int(c), int(0 if m is None else m)
        if not -2 ** 31 <= c < 2 ** 31 or not 0 <= m < 2 ** 31:
            raise ValueError('a class must fit int32 and a min_count lie in 0..2^31 - 1, got (%d, %d)' % (c, m))
        pairs.append((c, m))
    uniq = sorted(set(p for p in pairs if p is not None))
    index = {p: q for q, p in enumerate(uniq)}
    conds = np.asarray(uniq, dtype=np.int32).reshape(-1, 2)
    draw_cond = np.asarray([-1 if p is None else index[p] for p in pairs], dtype=np.int32)
    return conds, draw_cond


def window_label_counts(labels, window, cls):
    """Number of voxels equal to `cls` in every window of a label batch: labels N x D x H x W (uint8 / int32 / int64, views accepted),
    window (wd, wh, ww) -> int32 N x (D - wd + 1) x (H - wh + 1) x (W - ww + 1), exact.  Three separable passes on the device."""
    lab = _crop_labels(labels)
    N, D, H, W = (int(s) for s in lab.shape)
    win = _crop_window(window, (D, H, W))
    if D * H * W >= 2 ** 31:
        raise ValueError('a sample has %d voxels: the crop kernels take fewer than 2^31' % (D * H * W))
    out = torch.empty((N, D - win[0] + 1, H - win[1] + 1, W - win[2] + 1), dtype=torch.int32, device=lab.device)
    keep, wp3 = _int3_array(win)
    with torch.cuda.device(lab.device):
        wp, wn = _ws(nat.lib().da_window_label_counts_ws_bytes(N, D, H, W, wp3), lab)
        call('da_window_label_counts', ptr(lab), CROP_LABEL_DTYPE_CODE[lab.dtype], N, D, H, W, wp3, int(cls), ptr(out), wp, wn, stream())
    return out


def sample_crop_starts(labels, window, classes, min_counts, seed, sample0=0, include_last=False):
    """P crop starts per sample, drawn on the device with no host synchronisation.  labels N x D x H x W; classes / min_counts: one entry
    per draw (class None: no condition).  Per axis the domain is max(S - w, 1) starts (S - w + 1 with include_last); the admissible set A of
    a draw holds the starts of the domain, in raster order, whose window has >= min_count voxels of the class; with bits =
    hash(seed, (sample0 + n) * 65536 + p, CROP_STREAM) the result is element (bits * |A|) >> 32 of A.  An empty A yields the start with the
    largest count (first in raster order) and info[..., 0] = 0.  Returns (starts int32 N x P x 3 (z, y, x), info int32 N x P x 2 =
    (|A|, count at the chosen start; -1 for an unconditioned draw)), both on the device.  Sample n of a batch with sample0 = 0 equals sample
    0 of a call with sample0 = n."""
    lab = _crop_labels(labels)
    N, D, H, W = (int(s) for s in lab.shape)
    win = _crop_window(window, (D, H, W))
    if D * H * W >= 2 ** 31:
        raise ValueError('a sample has %d voxels: the crop kernels take fewer than 2^31' % (D * H * W))
    conds, draw_cond = crop_conditions(classes, min_counts)
    P = int(draw_cond.shape[0])
    sample0 = int(sample0)
    if sample0 < 0 or sample0 + N >= 2 ** 31:
        raise ValueError('sample0 must be >= 0 and sample0 + N below 2^31')
    dc = _const_tensor(draw_cond, lab.device)
    starts = torch.empty((N, P, 3), dtype=torch.int32, device=lab.device)
    info = torch.empty((N, P, 2), dtype=torch.int32, device=lab.device)
    keep, wp3 = _int3_array(win)
    Q = int(conds.shape[0])
    carr = nat.ctypes.cast((nat.ctypes.c_int * max(2 * Q, 1))(*[int(v) for v in conds.reshape(-1)]), nat.ctypes.c_void_p)
    with torch.cuda.device(lab.device):
        wp, wn = (None, 0) if Q == 0 else _ws(nat.lib().da_crop_sample_starts_ws_bytes(N, D, H, W, wp3, 1 if include_last else 0), lab)
        call('da_crop_sample_starts', ptr(lab), CROP_LABEL_DTYPE_CODE[lab.dtype], N, D, H, W, wp3, 1 if include_last else 0, P, carr, Q,
             ptr(dc), int(seed) & 0xFFFFFFFF, sample0, ptr(starts), ptr(info), wp, wn, stream())
    return starts, info


def crop_gather(image, labels, starts, window):
    """The crops of a batch at device-resident starts, one launch: image N x C x D x H x W float32, labels N x D x H x W (1-, 4- or 8-byte
    integers) or None, starts int32 N x P x 3 (z, y, x) -> ((N P) x C x wd x wh x ww, (N P) x wd x wh x ww in the labels' dtype), sample-major.
    A start outside [0, S - w] is clamped into it inside the kernel."""
    nat.require_cuda(image, labels, starts)
    if image.dim() != 5 or image.dtype != torch.float32:
        raise ValueError('image must be N x C x D x H x W float32')
    img = image.contiguous()
    N, C, D, H, W = (int(s) for s in img.shape)
    win = _crop_window(window, (D, H, W))
    if D * H * W >= 2 ** 31:
        raise ValueError('a sample has %d voxels: the crop kernels take fewer than 2^31' % (D * H * W))
    if starts.dim() != 3 or starts.shape[0] != N or starts.shape[2] != 3 or starts.dtype != torch.int32 or not 1 <= starts.shape[1] <= CROP_MAX_DRAWS:
        raise ValueError('starts must be int32 N x P x 3 with N = %d and 1 <= P <= %d' % (N, CROP_MAX_DRAWS))
    st = starts.contiguous()
    P = int(st.shape[1])
    lab = lab_out = None
    lb = 0
    if labels is not None:
        if tuple(labels.shape) != (N, D, H, W) or labels.dtype.is_floating_point or labels.element_size() not in (1, 4, 8):
            raise ValueError('labels must be integers of 1, 4 or 8 bytes, N x D x H x W = %s' % ((N, D, H, W),))
        lab = labels.contiguous()
        lb = lab.element_size()
        lab_out = torch.empty((N * P,) + win, dtype=lab.dtype, device=lab.device)
    out = torch.empty((N * P, C) + win, dtype=torch.float32, device=img.device)
    keep, wp3 = _int3_array(win)
    with torch.cuda.device(img.device):
        call('da_crop_gather', ptr(img), ptr(out), C, ptr(lab), ptr(lab_out), lb, ptr(st), N, P, D, H, W, wp3, stream())
    return out, lab_out


# ------------------------------------------------------------------------------------------------
# blended sliding-window inference (csrc/blend.hip; lib/inference.py SlidingWindowPredictor)
# ------------------------------------------------------------------------------------------------
BLEND_MAX_CLASSES = 256             # DA_BLEND_MAX_CLASSES (include/deepatlas_hip.h): labels are uint8
BLEND_FLIP_BITS = {'z': 1, 'y': 2, 'x': 4}      # bits of da_blend_accumulate's flip mask


def _blend_acc(acc):
    nat.require_cuda(acc)
    if acc.dim() != 4 or acc.dtype != torch.float32 or not acc.is_contiguous():
        raise ValueError('acc must be a contiguous float32 D x H x W x K tensor')
    if not 2 <= acc.shape[3] <= BLEND_MAX_CLASSES:
        raise ValueError('acc holds %d classes: 2 ... %d' % (acc.shape[3], BLEND_MAX_CLASSES))
    return tuple(int(s) for s in acc.shape)


def blend_accumulate(acc, tile_logits, tile0, tile, overlap, window, flip=0):
    """Adds the window-weighted softmax of a run of Partition's tiles into the accumulator of their volume, in place (da_blend_accumulate).
    acc D x H x W x K float32; tile_logits n x K x tz x ty x tx float32, the net's output for tiles tile0 ... tile0 + n - 1 of the raster tile
    order (channels-last memory, as the nets return it, is read without a copy); tile / overlap (z, y, x); window = three per-axis tables
    (lib.transforms.importance_window), uploaded once and kept by content; flip: BLEND_FLIP_BITS of the axes along which the tiles were
    mirrored before the net saw them.  Per voxel the covering tiles are added in ascending tile order, each add from the stored value: the
    result is bit-identical from run to run and for every split of the tiles into calls.  No autograd.  Returns acc."""
    import numpy as np
    D, H, W, K = _blend_acc(acc)
    if tile_logits.dim() != 5 or tile_logits.dtype != torch.float32 or tile_logits.shape[1] != K or tile_logits.device != acc.device:
        raise ValueError('tile_logits must be float32 n x %d x tz x ty x tx on the device of acc' % K)
    if len(tile) != 3 or len(overlap) != 3 or len(window) != 3:
        raise ValueError('tile, overlap and window take three entries each (z, y, x)')
    t3 = tuple(int(v) for v in tile)
    if tuple(int(s) for s in tile_logits.shape[2:]) != t3:
        raise ValueError('tile_logits holds tiles of %s, tile is %s' % (tuple(tile_logits.shape[2:]), t3))
    tabs = []
    for w, t in zip(window, t3):
        arr = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1))
        if arr.shape[0] != t:
            raise ValueError('a window table has %d entries, its tile axis %d' % (arr.shape[0], t))
        tabs.append(_const_tensor(arr, acc.device))
    a = ndhwc(tile_logits.detach())
    (k1, tp), (k2, op) = _int3_array(t3), _int3_array(overlap)
    with torch.cuda.device(acc.device):
        call('da_blend_accumulate', ptr(a), ptr(acc), D, H, W, K, tp, op, int(tile0), int(a.shape[0]), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]),
             int(flip), stream())
    return acc


def blend_finalize(acc, return_conf=False):
    """Label map of an accumulator (da_blend_finalize): acc D x H x W x K float32 -> uint8 D x H x W, the first-maximum argmax over the classes;
    with return_conf also float32 D x H x W, acc[label] / sum over the classes (NaN where a NaN logit reached the voxel)."""
    D, H, W, K = _blend_acc(acc)
    labels = torch.empty((D, H, W), dtype=torch.uint8, device=acc.device)
    conf = torch.empty((D, H, W), dtype=torch.float32, device=acc.device) if return_conf else None
    with torch.cuda.device(acc.device):
        call('da_blend_finalize', ptr(acc), D * H * W, K, ptr(labels), ptr(conf), stream())
    return (labels, conf) if return_conf else labels


# ------------------------------------------------------------------------------------------------
# applying a registration on the files' own grids (regapply.hip): the cubic B-spline prefilter and the warp through frames.  No autograd.
# ------------------------------------------------------------------------------------------------
BSPLINE_HORIZON = 24                # DA_BSPLINE_HORIZON (include/deepatlas_hip.h)
WARP_ORDERS = (0, 1, 3)
_PREFILTER_AXES = {0: 4, 1: 2, 2: 1}      # axis of a D x H x W volume -> bit of da_bspline3_prefilter's mask


def bspline_prefilter(vol, axes=(0, 1, 2)):
    """Cubic B-spline coefficients of a D x H x W or C x D x H x W device volume (float32, float64, int16, uint8 or int32), float32 of the same
    shape: scipy.ndimage.spline_filter(vol, 3, mode='mirror') (da_bspline3_prefilter: pole sqrt(3) - 2, gain 6 per axis, whole-sample mirror
    boundaries; an axis of extent 1 is left as it is).  axes: the axes of D, H, W (0, 1, 2) to filter, all three by default."""
    single = _volume4(vol)
    try:
        mask = sum(_PREFILTER_AXES[int(a)] for a in set(axes))
    except (KeyError, TypeError, ValueError):
        raise ValueError('axes takes a subset of (0, 1, 2) = (D, H, W), got %r' % (axes,))
    nat.require_cuda(vol)
    v = (vol.unsqueeze(0) if single else vol).contiguous()
    C, D, H, W = (int(s) for s in v.shape)
    out = torch.empty((C, D, H, W), dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        call('da_bspline3_prefilter', ptr(v), PREPROCESS_DTYPE_CODE[v.dtype], ptr(out), C, D, H, W, mask, stream())
    return out[0] if single else out


def _frame3(frame, what):
    """A frame ((a, b) per axis, (D, H, W) order; lib.inference.frame_of) -> six floats, checked."""
    import math
    try:
        flat = [float(v) for pair in frame for v in pair]
    except (TypeError, ValueError):
        flat = []
    if len(flat) != 6 or len(frame) != 3:
        raise ValueError('%s must hold three (a, b) pairs in (D, H, W) order, got %r' % (what, frame))
    if not all(math.isfinite(v) for v in flat) or any(flat[k] == 0.0 for k in (0, 2, 4)):
        raise ValueError('%s needs finite (a, b) with a != 0, got %r' % (what, frame))
    return flat


def warp_to_grid(moving, disp, out_size, fixed_frame, moving_frame, order=1, default=0, prefiltered=False, world=None):
    """A moving scan on its own grid carried onto a fixed scan's own grid through a field predicted on the prepared grid, with ONE
    interpolation (da_warp_frames).  moving: D x H x W or C x Dm x Hm x Wm device volume on the moving file's grid.  disp: 1 x 3 x Dp x Hp x Wp
    float32 in WarpFn's units (normalised, channel 0 = x).  out_size = (Do, Ho, Wo): the fixed file's grid.  fixed_frame / moving_frame:
    lib.inference.frame_of's pairs (a, b) per axis, native index = a * prepared index + b.  Output voxel x reads the moving volume at
    y = a_m (p + u(p)) + b_m with p = (x - b_f) / a_f and u sampled trilinearly under border padding; y outside [-0.5, n - 0.5) on any
    axis gives `default`.  order 0: nearest, the source dtype bit for bit (labels); 1: linear with edge-clamped taps, float32; 3: cubic
    B-spline over the coefficients of bspline_prefilter (computed here unless prefiltered=True says `moving` already holds them), float32, not
    clamped to the input's range.  A non-finite sample position gives NaN in a floating-point output and `default` in an integer one.
    world = (A_f, A_m), the two files' index-to-world affines (4 x 4 or 3 x 4, acting on (i, j, k) = (W, H, D) index): also returns the
    displacement in millimetres A_m (y, 1) - A_f (x, 1), float32 3 x Do x Ho x Wo (world x, y, z).  No autograd."""
    import math
    import numpy as np
    single = _volume4(moving, 'moving')
    if order not in WARP_ORDERS:
        raise ValueError('order %r: 0 (nearest), 1 (linear) or 3 (cubic B-spline)' % (order,))
    if not torch.is_tensor(disp) or disp.dim() != 5 or disp.shape[0] != 1 or disp.shape[1] != 3 or disp.dtype != torch.float32:
        raise ValueError('disp must be a 1 x 3 x D x H x W float32 displacement field, got %s'
                         % ((tuple(disp.shape), disp.dtype) if torch.is_tensor(disp) else type(disp),))
    if min(int(s) for s in disp.shape[2:]) < 2:
        raise ValueError('the displacement field needs >= 2 voxels per axis (align_corners=True), got %s' % (tuple(disp.shape),))
    if disp[0, 0].numel() >= 2 ** 29:
        raise ValueError('the displacement field has %d voxels: the warp takes fewer than 2^29' % disp[0, 0].numel())
    if len(out_size) != 3 or min(int(s) for s in out_size) < 1:
        raise ValueError('out_size takes three positive extents (D, H, W), got %r' % (out_size,))
    frames = _frame3(fixed_frame, 'fixed_frame') + _frame3(moving_frame, 'moving_frame')
    if prefiltered and order != 3:
        raise ValueError('prefiltered goes with order 3 only')
    if prefiltered and moving.dtype != torch.float32:
        raise ValueError('prefiltered coefficients are float32, got %s' % moving.dtype)
    integer = order == 0 and not moving.dtype.is_floating_point
    if integer:
        info = torch.iinfo(moving.dtype)
        if not math.isfinite(float(default)) or int(default) != default or not info.min <= int(default) <= info.max:
            raise ValueError('default %r is not a value of %s' % (default, moving.dtype))
    aff = None
    if world is not None:
        try:
            mats = [np.asarray(A, dtype=np.float64) for A in world]
        except (TypeError, ValueError):
            mats = []
        if len(mats) != 2 or any(A.shape not in ((4, 4), (3, 4)) or not np.isfinite(A).all() for A in mats):
            raise ValueError('world takes (A_f, A_m), two finite 4 x 4 or 3 x 4 index-to-world matrices')
        aff = (ctypes.c_double * 24)(*[float(v) for A in mats for v in A[:3].reshape(-1)])
    v = moving.unsqueeze(0) if single else moving
    C, Dm, Hm, Wm = (int(s) for s in v.shape)
    Do, Ho, Wo = (int(s) for s in out_size)
    if C * Do * Ho * Wo >= PREPROCESS_MAX_VOXELS:
        raise ValueError('the output has %d elements: the warp takes fewer than 2^31' % (C * Do * Ho * Wo))
    nat.require_cuda(v, disp)
    if v.device != disp.device:
        raise ValueError('moving and disp live on different devices')
    v = v.contiguous()
    if order == 3 and not prefiltered:
        v = bspline_prefilter(v)
    u = ndhwc(disp.detach())
    Dp, Hp, Wp = (int(s) for s in u.shape[1:4])
    out = torch.empty((C, Do, Ho, Wo), dtype=v.dtype if order == 0 else torch.float32, device=v.device)
    wd = torch.empty((3, Do, Ho, Wo), dtype=torch.float32, device=v.device) if world is not None else None
    with torch.cuda.device(v.device):
        call('da_warp_frames', ptr(v), PREPROCESS_DTYPE_CODE[v.dtype], ptr(u), ptr(out), ptr(wd), C, Dm, Hm, Wm, Dp, Hp, Wp, Do, Ho, Wo,
             (ctypes.c_double * 12)(*frames), aff, int(order), float(default), stream())
    out = out[0] if single else out
    return (out, wd) if world is not None else out
