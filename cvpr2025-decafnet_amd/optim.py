"""The Trainer's parameter update (libs/worker_v2.py:318-325, :647-656; libs/modeling/optim.py) on the GPU's multi-tensor kernels.

    clip_grad_norm_ -> dcf_optim_grad_norm (+ dcf_optim_scale stand-alone, or the coefficient folded into the update)
    StepGuard       -> dcf_guard_grad_norm / dcf_guard_adam_step: the same two launches, skipped on the device if a gradient is non-finite
    AdamW.step()    -> dcf_optim_adam_step: one launch over every parameter tensor, the decay / no-decay groups by value
    device_count    -> dcf_clock_adam_step: the same launch with Adam's step counts and bias corrections read on the device
    _ema_update()   -> the same launch (``attach_ema``)
    scheduler       -> LinearWarmupMultiStepLR / LinearWarmupCosineAnnealingLR: host arithmetic in double, a closed form per step

No arithmetic on tensors happens in this module: the host builds the device table of addresses (include/decafnet_hip.h,
dcf_optim_row) and launches.  Nothing waits on the host.  There is no CPU path.
"""
import copy
import ctypes
import math

import numpy as np
import torch

from . import _lib

CHUNK = _lib.OPTIM_CHUNK

# dcf_optim_row as a packed numpy record (64 bytes)
_ROW = np.dtype([('p', '<u8'), ('g', '<u8'), ('exp_avg', '<u8'), ('exp_avg_sq', '<u8'), ('ema', '<u8'), ('n', '<i8'),
                 ('group', '<i4'), ('flags', '<i4'), ('chunk0', '<i8')])
assert _ROW.itemsize == 64


def _check_tensor(t, what):
    """fp32, contiguous (dense): what the kernels address.  The device is checked where a kernel is about to run."""
    if not torch.is_tensor(t):
        raise TypeError(f'{what}: a tensor is expected, got {type(t).__name__}')
    if t.dtype != torch.float32:
        raise ValueError(f'{what} must be float32 (got {t.dtype})')
    if t.layout != torch.strided or not t.is_contiguous():
        raise ValueError(f'{what} must be contiguous (shape {tuple(t.shape)}, strides {tuple(t.stride())})')


def _need_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'{what} is on {t.device}: the update runs on the GPU only (call model.cuda() first; there is no CPU path)')


class _Table:
    """The device table of one list of tensors and its chunk map.  ``update(rows)`` uploads only when the host copy changed."""

    def __init__(self):
        self.host = self.device = None
        self.rows = self.chunk_map = None
        self.n_tensors = self.n_chunks = 0
        self.uploads = 0

    def update(self, rec, device):
        counts = -(-rec['n'] // CHUNK)
        rec['chunk0'] = np.cumsum(counts) - counts
        if self.host is not None and self.device == device and self.host.tobytes() == rec.tobytes():
            return self
        cmap = np.repeat(np.arange(len(rec), dtype=np.int32), counts)
        # pinned staging + non_blocking: the copies are ordered on the current stream and the host does not wait for them
        # (the pinned blocks go back to torch's host allocator, which reuses them only after the copy has run)
        up = lambda a: torch.from_numpy(a).pin_memory().to(device, non_blocking=True)
        self.rows = up(rec.view(np.uint8).reshape(-1).copy()) if len(rec) else None
        self.chunk_map = up(cmap) if len(cmap) else None
        self.host, self.device, self.n_tensors, self.n_chunks = rec.copy(), device, len(rec), int(len(cmap))
        self.uploads += 1
        return self

    def args(self):
        return _lib.ptr(self.rows), _lib.ptr(self.chunk_map), self.n_tensors, self.n_chunks


def _grad_records(params, what='parameter'):
    """one record per tensor of `params` that has a gradient (p = 0: only g is read) -> (records, device or None)"""
    params = [params] if torch.is_tensor(params) else params
    f32, ptrs, sizes, device = torch.float32, [], [], None
    for i, p in enumerate(params):
        g = p.grad
        if g is None:
            continue
        if device is None:
            _need_gpu(g, f'the gradient of {what} {i}')
            device = g.device
        if g.dtype is not f32 or g.device != device or not g.is_contiguous():
            _check_tensor(g, f'the gradient of {what} {i}')
            raise ValueError(f'the gradient of {what} {i} is on {g.device}, the first on {device}: one device')
        ptrs.append(g.data_ptr())
        sizes.append(g.numel())
    rec = np.zeros(len(ptrs), dtype=_ROW)
    rec['g'], rec['n'] = ptrs, sizes
    return rec, device


_CLIP_TABLE = _Table()


def _mark_written(tensors):
    """The kernels write through raw addresses, which torch cannot see: bump the in-place version counter of every tensor a launch
    wrote, as an in-place torch op would have.  The forward engine re-binds and re-finalises its repacked / folded weights by
    (address, version) of each parameter (modeling._Engine.bind), and autograd checks saved tensors by it.  No arithmetic, no host wait."""
    if tensors:
        torch.autograd.graph.increment_version(tensors)


def _norm_launch(table, max_norm, device, guard=None):
    out = torch.empty(2, dtype=torch.float32, device=device)
    lib = _lib.lib()
    outs = (ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr() + 4))
    with torch.cuda.device(device):
        if guard is None:
            _lib.check(lib.dcf_optim_grad_norm(*table.args(), float(max_norm or 0.0), *outs, _lib.current_stream()), 'dcf_optim_grad_norm')
        else:
            _lib.check(lib.dcf_guard_grad_norm(*table.args(), float(max_norm or 0.0), *outs, guard._on(device), _lib.current_stream()),
                       'dcf_guard_grad_norm')
    return out[0], out[1]


# dcf_guard_state as a packed numpy record (48 bytes)
_GUARD = np.dtype([('verdict', '<i4'), ('first_bad_row', '<i4'), ('n_bad_rows', '<i4'), ('reserved0', '<i4'), ('applied', '<i8'),
                   ('skipped', '<i8'), ('last_skipped_attempt', '<i8'), ('conv_flag', '<i4'), ('reserved1', '<i4')])
assert _GUARD.itemsize == ctypes.sizeof(_lib.DcfGuardState) == 48


class StepGuard:
    """Owns one dcf_guard_state record on ``device`` (include/decafnet_hip_guard.h): the verdict of the last guarded norm and the
    running counts of applied and skipped steps.  Hand it to ``grad_norm_and_coef(..., guard=g)`` and to ``AdamW.step(..., guard=g)``:
    the norm decides on the GPU whether any gradient is non-finite, the update reads the decision there and writes nothing on a skip.
    Neither call reads anything back.  ``arm()`` ... ``disarm()`` around the forward, the backward and the update keeps the
    conv-gradient operators' sticky numerics word from failing the next call; the guarded norm turns it into a skip instead.
    ``report()`` is the only host read, for logs and checkpoints."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'StepGuard on {device}: the guarded update runs on the GPU only (there is no CPU path)')
        self.device = device if device.index is not None else torch.device('cuda', torch.cuda.current_device())
        self._state = torch.empty(_GUARD.itemsize // 8, dtype=torch.int64, device=self.device)         # 8-byte aligned
        self._rows = None                               # per row of the last guarded norm's table: the index into its `parameters`
        self.armed = False
        self.load_counters(0, 0)

    def _on(self, device):
        if device != self.device:
            raise ValueError(f'the guard lives on {self.device}, the tensors on {device}: one device')
        return ctypes.c_void_p(self._state.data_ptr())

    def load_counters(self, applied, skipped):
        """reset the record to `applied` applied and `skipped` skipped steps and nothing known about the last skip (stream-ordered)"""
        rec = np.zeros(1, dtype=_GUARD)
        rec['first_bad_row'], rec['last_skipped_attempt'], rec['applied'], rec['skipped'] = -1, -1, int(applied), int(skipped)
        with torch.cuda.device(self.device):
            self._state.copy_(torch.from_numpy(rec.view(np.int64).reshape(-1).copy()).pin_memory(), non_blocking=True)
        return self

    def arm(self):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dcf_guard_arm(self._on(self.device), _lib.current_stream()), 'dcf_guard_arm')
        self.armed = True
        return self

    def disarm(self):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().dcf_guard_disarm(_lib.current_stream()), 'dcf_guard_disarm')
        self.armed = False
        return self

    def report(self, names=None):
        """Reads the record back (THE host read: it waits for the stream).  -> {'applied', 'skipped', 'last_skipped_attempt' (attempts
        count from 0; -1: none yet), 'first_bad', 'n_bad_rows', 'conv_flag', 'verdict'}.  'first_bad' is the first tensor with a
        non-finite chunk sum at the last skipped attempt: its entry of ``names`` (aligned with the ``parameters`` the guarded norm was
        given) if names are given, else its row in the norm's table (the tensors that had a gradient, in order); None if no step was
        skipped yet or the conv-gradient word alone caused the skip.  'verdict' is that of the last norm (0 apply, 1 skip)."""
        rec = self._state.cpu().numpy().view(_GUARD)[0]
        row = int(rec['first_bad_row'])
        first = None
        if row >= 0:
            first = row
            if names is not None:
                names = list(names)
                i = self._rows[row] if self._rows is not None and row < len(self._rows) else row
                first = names[i] if i < len(names) else row
        return {'applied': int(rec['applied']), 'skipped': int(rec['skipped']), 'last_skipped_attempt': int(rec['last_skipped_attempt']),
                'first_bad': first, 'n_bad_rows': int(rec['n_bad_rows']), 'conv_flag': int(rec['conv_flag']), 'verdict': int(rec['verdict'])}


def bias_correction_table(b1, b2, max_len=_lib.CLOCK_MAX_TABLE):
    """The bias corrections of Adam for the step counts t = 1, 2, ... as a float32 array (n, 2): row t - 1 holds 1 - b1^t and
    sqrt(1 - b2^t), computed in double exactly as ``AdamW._group_array`` computes the pair it passes by value, then rounded to fp32
    as a C float assignment rounds.  The last row is the first whose two floats are both 1.0: from there on the corrections do not
    change, and dcf_clock_adam_step (include/decafnet_hip_clock.h) takes 1.0 for every count past the end.  Betas so close to 1 that
    this takes more than ``max_len`` rows are refused."""
    b1, b2 = float(b1), float(b2)
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f'bias_correction_table: betas ({b1}, {b2}) must lie in [0, 1)')
    # 1 - x rounds to 1.0f once x <= 2^-25, sqrt(1 - x) no later: the length is about 25 ln 2 / -ln b.  Estimated first, so that a
    # hopeless pair is refused at once and not after max_len powers.
    b = max(b1, b2)
    too_long = ValueError(f'betas ({b1}, {b2}): the bias corrections reach 1.0 in fp32 only after more than {max_len} steps; '
                          f'device_count=True keeps a table of them and takes at most that many')
    if b > 0.0 and 25.0 * math.log(2.0) / -math.log(b) > 1.01 * max_len:
        raise too_long
    one = np.float32(1.0)
    rows, t = [], 0
    while True:
        t += 1
        if t > max_len:
            raise too_long
        pair = (np.float32(1.0 - b1 ** t), np.float32(math.sqrt(1.0 - b2 ** t)))
        rows.append(pair)
        if pair[0] == one and pair[1] == one:
            return np.array(rows, dtype=np.float32).reshape(-1, 2)


def grad_norm_and_coef(parameters, max_norm, _table=None, guard=None):
    """(total L2 norm of the gradients, min(1, max_norm / (norm + 1e-6))) as two 0-d device tensors, for the fused path:
    ``optimizer.step(clip_coef=coef)`` folds the coefficient into the update and leaves ``p.grad`` unscaled.  max_norm <= 0 or None
    gives the coefficient 1.  The norm is summed in a fixed order: the same gradients give the same bits on every run.
    ``guard``: a ``StepGuard``.  The norm then also decides, on the GPU, whether the step may be applied (dcf_guard_grad_norm): with
    finite gradients norm and coefficient have the bits of the unguarded call; with a NaN, an inf or a chunk whose squares overflow
    fp32 anywhere the coefficient is +0, the norm stays non-finite and the guard's verdict is skip.  One attempt is counted per call."""
    table = _CLIP_TABLE if _table is None else _table
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)      # once: a generator is consumed by the first walk
    rec, device = _grad_records(params)
    if device is None:                                                              # no gradient anywhere: the norm is 0
        for i, p in enumerate(params):
            _need_gpu(p, f'parameter {i}')
        device = params[0].device if params else torch.device('cuda')
    table.update(rec, device)
    if guard is not None:
        guard._rows = [i for i, p in enumerate(params) if p.grad is not None]
    return _norm_launch(table, max_norm, device, guard)


def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_ for norm_type = 2: scales every gradient in place by min(1, max_norm / (norm + 1e-6)) and
    returns the norm (before the scaling) as a device tensor."""
    parameters = [parameters] if torch.is_tensor(parameters) else list(parameters)
    norm, coef = grad_norm_and_coef(parameters, max_norm)
    table = _CLIP_TABLE
    if table.n_chunks:
        with torch.cuda.device(norm.device):
            _lib.check(_lib.lib().dcf_optim_scale(*table.args(), _lib.ptr(coef), _lib.current_stream()), 'dcf_optim_scale')
        _mark_written([p.grad for p in parameters if p.grad is not None])
    return norm


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (mode='adamw') / torch.optim.Adam (mode='adam': the weight decay added to the gradient) as ONE kernel launch
    per step over every parameter tensor of every group.  ``param_groups`` and ``state`` are torch's (``state[p] = {step, exp_avg,
    exp_avg_sq}``, the same group keys), so torch's schedulers drive it and ``state_dict()`` moves between the two in both
    directions.  lr, weight_decay, betas and eps are read from the groups at every step and travel by value with the launch.

    ``step(clip_coef=None)``: clip_coef is the one-element device tensor of ``grad_norm_and_coef`` (or None): the gradient is
    multiplied by it inside the update, ``p.grad`` itself keeps its values.  ``attach_ema`` makes the same launch move an EMA copy.
    ``step(guard=g)``: the launch obeys the verdict of the ``StepGuard``'s last ``grad_norm_and_coef(..., guard=g)``: on a skip it
    writes no byte of any parameter, moment or EMA tensor.  The host cannot know the verdict, so ``state[p]['step']`` advances
    either way: the bias corrections follow the attempted steps.

    ``device_count=True`` (include/decafnet_hip_clock.h, dcf_clock_adam_step) moves the step counts to the GPU: one int64 tensor holds
    the count of every parameter of every group in table order, made at the first step and laid out again when a group is added.  The
    launch reads a row's count t - 1, takes 1 - b1^t and sqrt(1 - b2^t) from a table that ``bias_correction_table`` built on the host
    from the very doubles the default path rounds (one table per distinct betas, uploaded once), and a second tiny kernel advances the
    counts of the rows that had a gradient -- under a guard only where the update was applied, so the corrections follow APPLIED
    steps as with ``torch.cuda.amp.GradScaler``.  Finite gradients give the bits of the default path.  ``state[p]['step']`` is not
    read by ``step()`` and goes stale between checkpoints; ``state_dict()`` reads the counts back (a host read, like the checkpoint
    itself) and hands out torch's format, ``load_state_dict()`` uploads them: a state dict moves freely between the two settings
    and torch.optim.AdamW.  Every parameter may have a count of its own: the limit of 8 (group, count) pairs per launch is gone, the
    limit of 8 parameter groups stays.  ``False`` -- the default -- launches exactly what it launched before the option existed.
    Parameters are fp32, contiguous and, when ``step`` runs, on the GPU."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, mode='adamw', device_count=False):
        if mode not in _lib.OPTIM_MODES:
            raise ValueError(f"mode must be 'adamw' or 'adam' (got {mode!r})")
        if not isinstance(device_count, bool):
            raise ValueError(f'device_count = {device_count!r} (True or False)')
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f'invalid hyper-parameters: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}')
        # torch's own group keys (torch/optim/adam.py), so that a state dict is interchangeable; the switches this class does not
        # implement must keep these values
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=mode == 'adamw')
        self._table = _Table()
        self._ema, self._ema_beta = {}, None
        self._decoupled = mode == 'adamw'            # for groups loaded from a state dict that lacks torch's decoupled_weight_decay key
        # device_count: the counts on the device in the order of `_layout` (None: not laid out yet; `_host_counts` {parameter: count}
        # then holds what was loaded or read back last), the uploaded tables by betas, and the launch's two host arrays
        self.device_count = device_count
        self._steps = self._layout = None
        self._host_counts, self._bc, self._bc_args = {}, {}, (None, None, None)
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        g = len(self.param_groups) - 1
        for i, p in enumerate(self.param_groups[g]['params']):
            _check_tensor(p, self._name(g, i, p))

    def _name(self, g, i, p):
        names = self.param_groups[g].get('param_names')
        return f"parameter {names[i]!r}" if names else f"parameter {i} of group {g} (shape {tuple(p.shape)})"

    @property
    def table_uploads(self):
        """how often the device table was (re)built: it is rebuilt only when an address, a size or a group in it changed"""
        return self._table.uploads

    def attach_ema(self, ema, beta):
        """Make step() also update an EMA copy: ema <- lerp(p_new, ema, beta) (Trainer._ema_update, worker_v2.py:654-656) for every
        optimizer parameter that has a partner, gradient or not.  ``ema``: a ModelEma, a {parameter: tensor} dict, or a sequence of
        tensors aligned with the parameters of all groups in order.  ``attach_ema(None, None)`` detaches."""
        if ema is None:
            self._ema, self._ema_beta = {}, None
            return self
        if isinstance(ema, ModelEma):
            pairs = dict(ema.pairs())
        elif isinstance(ema, dict):
            pairs = dict(ema)
        else:
            flat = [p for g in self.param_groups for p in g['params']]
            ema = list(ema)
            if len(ema) != len(flat):
                raise ValueError(f'{len(ema)} EMA tensors for {len(flat)} parameters')
            pairs = dict(zip(flat, ema))
        beta = float(beta)
        if not 0.0 <= beta <= 1.0:
            raise ValueError(f'beta = {beta} must lie in [0, 1]')
        mine = {}
        for g, group in enumerate(self.param_groups):
            for i, p in enumerate(group['params']):
                e = pairs.get(p)
                if e is None:
                    continue
                _check_tensor(e, f'the EMA copy of {self._name(g, i, p)}')
                if e.shape != p.shape:
                    raise ValueError(f'the EMA copy of {self._name(g, i, p)} has shape {tuple(e.shape)}, not {tuple(p.shape)}')
                mine[p] = e
        self._ema, self._ema_beta = mine, beta
        return self

    def _bad(self, g, i, p, t, what, device):
        """the message for a tensor of parameter i of group g that the kernel cannot address (the checks of the hot loop, spelt out)"""
        _check_tensor(t, f'{what} of {self._name(g, i, p)}')
        raise ValueError(f'{what} of {self._name(g, i, p)}: {tuple(t.shape)} on {t.device}, expected {tuple(p.shape)} on {device}')

    def _group_array(self, keys):
        """the dcf_optim_group records of the (parameter group, step count) pairs `keys`: the bias corrections depend on the count,
        which torch keeps per parameter (a parameter without a gradient does not advance)"""
        if len(keys) > _lib.OPTIM_MAX_GROUPS:
            raise NotImplementedError(f'{len(keys)} distinct (parameter group, step count) pairs in one step; one launch takes '
                                      f'{_lib.OPTIM_MAX_GROUPS}')
        arr = (_lib.DcfOptimGroup * max(len(keys), 1))()
        for (gi, t), k in keys.items():
            group = self.param_groups[gi]
            if group.get('amsgrad') or group.get('maximize'):
                raise NotImplementedError('amsgrad / maximize are not implemented')
            b1, b2 = (float(b) for b in group['betas'])
            h = arr[k]
            h.lr, h.weight_decay, h.b1, h.b2, h.eps = float(group['lr']), float(group['weight_decay']), b1, b2, float(group['eps'])
            h.one_minus_b1, h.one_minus_b2 = 1.0 - b1, 1.0 - b2                   # in double on the host, like the bias corrections
            h.bc1, h.sqrt_bc2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
            h.mode = _lib.OPTIM_MODES['adamw' if group.get('decoupled_weight_decay', self._decoupled) else 'adam']
        return arr

    # ---- device_count=True: the counts and the bias-correction tables on the device
    def _counts_on_host(self):
        """-> {parameter: count}.  Reads the device counts back if there are any (a host read: it waits for the stream)."""
        if self._steps is not None:
            self._host_counts = dict(zip(self._layout, self._steps.cpu().tolist()))
        return self._host_counts

    def _lay_counts(self, flat, device):
        """the int64 count tensor for the parameters `flat` (table order) on `device`: the known counts, 0 for a new parameter;
        uploaded stream-ordered from pinned memory"""
        known = self._counts_on_host()
        host = torch.tensor([int(known.get(p, 0)) for p in flat], dtype=torch.int64)
        with torch.cuda.device(device):
            self._steps = host.pin_memory().to(device, non_blocking=True)
        self._layout = list(flat)

    def _clock_args(self, device):
        """(groups, bc_tables, bc_len) of dcf_clock_adam_step: one record and one table per PARAMETER group"""
        n = len(self.param_groups)
        if n > _lib.OPTIM_MAX_GROUPS:
            raise NotImplementedError(f'{n} parameter groups; one launch takes {_lib.OPTIM_MAX_GROUPS}')
        groups = self._group_array({(g, 1): g for g in range(n)})       # bc1 / sqrt_bc2 of these records are ignored by the export
        betas = tuple((float(g['betas'][0]), float(g['betas'][1]), device) for g in self.param_groups)
        if self._bc_args[0] != betas:
            for key in betas:
                if key not in self._bc:
                    tab = bias_correction_table(key[0], key[1])
                    with torch.cuda.device(device):
                        self._bc[key] = (torch.from_numpy(tab.reshape(-1).copy()).pin_memory().to(device, non_blocking=True), len(tab))
            self._bc_args = (betas, (ctypes.c_void_p * n)(*[self._bc[k][0].data_ptr() for k in betas]),
                             (ctypes.c_int32 * n)(*[self._bc[k][1] for k in betas]))
        return groups, self._bc_args[1], self._bc_args[2]

    @torch.no_grad()
    def step(self, closure=None, clip_coef=None, guard=None):
        if closure is not None:
            raise NotImplementedError('step(closure) is not implemented')
        # One pass over the parameters gathers the table's columns as plain lists (this loop is the host cost of a step: a few calls
        # per tensor, no tensor arithmetic).  While the optimizer runs, state[p]['step'] is a Python number; state_dict() hands out
        # torch's one-element tensors.
        f32, state, ema_of = torch.float32, self.state, self._ema
        cp, cg, cm, cv, ce, cn, ck, cf = [], [], [], [], [], [], [], []
        keys, device, counts, written = {}, None, [], []
        on_device, flat = self.device_count, []
        for g, group in enumerate(self.param_groups):
            for i, p in enumerate(group['params']):
                if on_device:
                    flat.append(p)
                if device is None:
                    _need_gpu(p, self._name(g, i, p))
                    device = p.device
                elif p.device != device:
                    _need_gpu(p, self._name(g, i, p))
                    raise ValueError(f'{self._name(g, i, p)} is on {p.device}, the first parameter on {device}: one device per optimizer')
                cp.append(p.data_ptr())
                cn.append(p.numel())
                grad = p.grad
                if grad is None:
                    cg.append(0), cm.append(0), cv.append(0), ck.append(0), cf.append(_lib.OPTIM_NO_GRAD)
                else:
                    st = state[p]
                    if not st:
                        st['step'] = 0.0
                        st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    m, v = st['exp_avg'], st['exp_avg_sq']
                    for t, what in ((grad, 'the gradient'), (m, 'exp_avg'), (v, 'exp_avg_sq')):
                        if t.dtype is not f32 or t.device != device or t.shape != p.shape or not t.is_contiguous():
                            self._bad(g, i, p, t, what, device)
                    written.append(p)
                    cg.append(grad.data_ptr()), cm.append(m.data_ptr()), cv.append(v.data_ptr()), cf.append(0)
                    if on_device:                                # the count is the device's: the row names its parameter group alone
                        counts.append((st, None))
                        ck.append(g)
                    else:
                        t = float(st['step']) + 1
                        counts.append((st, t))                   # committed below, once nothing can raise any more
                        ck.append(keys.setdefault((g, t), len(keys)))
                e = ema_of.get(p) if ema_of else None
                if e is None:
                    ce.append(0)
                else:
                    if e.device != device:
                        raise ValueError(f'the EMA copy of {self._name(g, i, p)} is on {e.device}, the parameter on {device}')
                    ce.append(e.data_ptr())
                    written.append(e)
        if device is None:
            return None
        if on_device:
            groups, bc_tables, bc_len = self._clock_args(device)
        else:
            groups = self._group_array(keys)
        rec = np.zeros(len(cp), dtype=_ROW)
        for name, col in (('p', cp), ('g', cg), ('exp_avg', cm), ('exp_avg_sq', cv), ('ema', ce), ('n', cn), ('group', ck), ('flags', cf)):
            rec[name] = col
        if clip_coef is not None:
            _check_tensor(clip_coef, 'clip_coef')
            if clip_coef.numel() != 1 or clip_coef.device != device:
                raise ValueError(f'clip_coef: one float32 on {device} is expected')
        self._table.update(rec, device)
        ema = (int(bool(self._ema)), float(self._ema_beta or 0.0))
        if on_device and (self._steps is None or self._steps.device != device or len(flat) != len(self._layout)
                          or not all(a is b for a, b in zip(flat, self._layout))):
            self._lay_counts(flat, device)
        with torch.cuda.device(device):
            if on_device:                                        # the counts advance on the device, where the update is applied
                _lib.check(_lib.lib().dcf_clock_adam_step(*self._table.args(), ctypes.cast(groups, ctypes.c_void_p), len(self.param_groups),
                                                          ctypes.cast(bc_tables, ctypes.c_void_p), ctypes.cast(bc_len, ctypes.c_void_p),
                                                          _lib.ptr(self._steps), _lib.ptr(clip_coef),
                                                          None if guard is None else guard._on(device), *ema, _lib.current_stream()),
                           'dcf_clock_adam_step')
            elif guard is None:
                _lib.check(_lib.lib().dcf_optim_adam_step(*self._table.args(), ctypes.cast(groups, ctypes.c_void_p), len(keys),
                                                          _lib.ptr(clip_coef), *ema, _lib.current_stream()), 'dcf_optim_adam_step')
            else:                                                # the verdict of the guard's last norm decides on the device
                _lib.check(_lib.lib().dcf_guard_adam_step(*self._table.args(), ctypes.cast(groups, ctypes.c_void_p), len(keys),
                                                          _lib.ptr(clip_coef), guard._on(device), *ema, _lib.current_stream()),
                           'dcf_guard_adam_step')
        for st, t in counts:                                     # the update is enqueued: now the counts advance
            if t is not None:
                st['step'] = t
            written.append(st['exp_avg']), written.append(st['exp_avg_sq'])
        _mark_written(written)
        return None

    def state_dict(self):
        """torch's format: state[i] = {step (a one-element fp32 tensor on the CPU, as torch.optim.AdamW keeps it), exp_avg, exp_avg_sq}"""
        if self.device_count:                                    # the one host read: state[p]['step'] is brought up to date here alone
            known = self._counts_on_host()
            for p, st in self.state.items():
                if st:
                    st['step'] = float(known.get(p, 0))
        sd = super().state_dict()
        sd['state'] = {k: {**v, 'step': v['step'] if torch.is_tensor(v['step']) else torch.tensor(float(v['step']), dtype=torch.float32)}
                       for k, v in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if 'step' in st:
                st['step'] = float(st['step'])
        if self.device_count:                                    # the loaded counts replace the device's, for every parameter
            self._steps = self._layout = None
            self._host_counts = {p: int(st['step']) for p, st in self.state.items() if 'step' in st}
            flat = [p for g in self.param_groups for p in g['params']]
            if flat and flat[0].is_cuda:                         # else the first step uploads them
                self._lay_counts(flat, flat[0].device)


class ModelEma:
    """The Trainer's ``model_ema`` (worker_v2.py:225, :647-656): a deep copy of the model in eval() with requires_grad_(False),
    which every checkpoint is evaluated from.  ``attach(optimizer)`` makes the optimizer's launch update it; ``state_dict()`` is
    what goes under 'model_ema'."""

    def __init__(self, model, beta=0.999):
        self.model, self.beta = model, float(beta)
        memo = {}
        for m in model.modules():                 # what a forward left behind is not part of the copy: the bound engine (a native
            for k in ('_engine', '_out_cache', '_last_inputs', '_last_flat'):     # handle), the borrowed input and output buffers
                if m.__dict__.get(k) is not None:
                    memo[id(m.__dict__[k])] = {} if k == '_out_cache' else None
        self.module = copy.deepcopy(model, memo).eval().requires_grad_(False)

    def pairs(self):
        return list(zip(self.model.parameters(), self.module.parameters()))

    @torch.no_grad()
    def init_from(self, model=None):
        """Trainer._ema_init: copy the parameters and the buffers"""
        model = self.model if model is None else model
        for p, e in zip(model.parameters(), self.module.parameters()):
            e.copy_(p.detach())
        for b, e in zip(model.buffers(), self.module.buffers()):
            e.copy_(b.detach())
        return self

    def attach(self, optimizer):
        optimizer.attach_ema(self, self.beta)
        return self

    def state_dict(self):
        return self.module.state_dict()

    def load_state_dict(self, sd):
        return self.module.load_state_dict(sd)


def split_decay(model):
    """-> (decay, no_decay): the sorted parameter names of the reference's two groups (libs/modeling/optim.py:66-118).  Biases,
    the weights / scales of LayerNorm, Scale and LayerScale and ``bkgd_token`` are not decayed; the weights of nn.Linear, nn.Conv1d and
    MaskedConv1D are."""
    from torch import nn
    from . import modeling as M
    decayed = (nn.Linear, nn.Conv1d, M.MaskedConv1D, nn.Conv2d)
    plain = (M.LayerNorm, M.Scale, M.LayerScale, nn.LayerNorm, nn.Embedding, nn.BatchNorm2d, nn.BatchNorm3d)
    decay, no_decay = set(), set()
    for mn, m in model.named_modules():
        for pn, p in m.named_parameters(recurse=False):
            if not p.requires_grad:
                continue
            full = f'{mn}.{pn}' if mn else pn
            if pn.endswith('bias'):
                no_decay.add(full)
            elif pn.endswith('weight') and isinstance(m, decayed):
                decay.add(full)
            elif pn.endswith(('weight', 'scale')) and isinstance(m, plain):
                no_decay.add(full)
            elif pn.endswith('bkgd_token'):
                no_decay.add(full)
    named = {n for n, p in model.named_parameters() if p.requires_grad}
    both, neither = decay & no_decay, named - (decay | no_decay)
    assert not both, f'split_decay: {sorted(both)} fall under two rules (decayed and not decayed)'
    assert not neither, f'split_decay: no rule covers {sorted(neither)}'
    return sorted(decay), sorted(no_decay)


def make_optimizer(model, opt, device_count=False):
    """libs/modeling/optim.py:66-239 for ``opt = opt['optimizer']``: {name: 'adamw' | 'adam', lr, weight_decay}.  ``device_count``:
    the option of ``AdamW`` -- the step counts on the GPU."""
    name = opt['name']
    if name not in ('adamw', 'adam'):
        raise NotImplementedError(f"optimizer {name!r} is not implemented ('adamw' and 'adam' are)" if name == 'sgd'
                                  else f"unknown optimizer {name!r} ('adamw' and 'adam' are implemented)")
    decay, no_decay = split_decay(model)
    named = dict(model.named_parameters())
    for n in decay + no_decay:
        _check_tensor(named[n], f'parameter {n!r}')
    groups = [{'params': [named[n] for n in decay], 'weight_decay': opt['weight_decay'], 'lr': opt['lr']},
              {'params': [named[n] for n in no_decay], 'weight_decay': 0.0, 'lr': opt['lr']}]
    return AdamW(groups, lr=opt['lr'], betas=(0.9, 0.999), weight_decay=opt.get('weight_decay', 0), mode=name, device_count=device_count)


class _ClosedFormLR(torch.optim.lr_scheduler.LRScheduler):
    """a schedule given as a function of the step count (``_lr_at``), evaluated in double on the host at every step"""

    def _lr_at(self, k, base_lr):
        raise NotImplementedError

    def get_lr(self):
        return [self._lr_at(self.last_epoch, b) for b in self.base_lrs]

    _get_closed_form_lr = get_lr

    def _warmup(self, k, base_lr):
        """the linear ramp both schedules start with: warmup_start_lr at step 0, base_lr at steps warmup_epochs - 1 and warmup_epochs
        -> the value, or None past it"""
        w = self.warmup_epochs
        if k == w:
            return base_lr
        if k == 0:
            return self.warmup_start_lr
        if k < w:
            return self.warmup_start_lr + k * ((base_lr - self.warmup_start_lr) / (w - 1))
        return None


class LinearWarmupMultiStepLR(_ClosedFormLR):
    """Linear warm-up over ``warmup_epochs`` steps, then base_lr times ``gamma`` for every milestone passed, a milestone m taking
    effect at step warmup_epochs + m (m >= 1; the reference's chained form never applies one at or before the end of the warm-up)."""

    def __init__(self, optimizer, warmup_epochs, milestones, warmup_start_lr=0.0, gamma=0.1, last_epoch=-1):
        self.warmup_epochs, self.warmup_start_lr = int(warmup_epochs), warmup_start_lr
        self.milestones, self.gamma = tuple(sorted(int(m) for m in milestones)), gamma
        super().__init__(optimizer, last_epoch)

    def _lr_at(self, k, base_lr):
        lr = self._warmup(k, base_lr)
        if lr is None:
            lr = base_lr
            for m in self.milestones:
                if 0 < m <= k - self.warmup_epochs:
                    lr = lr * self.gamma
        return lr


class LinearWarmupCosineAnnealingLR(_ClosedFormLR):
    """Linear warm-up over ``warmup_epochs`` steps, then half a cosine from base_lr down to ``eta_min`` at step ``max_epochs``
    (and on along the same cosine past it)."""

    def __init__(self, optimizer, warmup_epochs, max_epochs, warmup_start_lr=0.0, eta_min=1e-8, last_epoch=-1):
        self.warmup_epochs, self.max_epochs = int(warmup_epochs), int(max_epochs)
        self.warmup_start_lr, self.eta_min = warmup_start_lr, eta_min
        super().__init__(optimizer, last_epoch)

    def _lr_at(self, k, base_lr):
        lr = self._warmup(k, base_lr)
        if lr is None:
            w, n = self.warmup_epochs, self.max_epochs - self.warmup_epochs
            lr = self.eta_min + (base_lr - self.eta_min) * (1 + math.cos(math.pi * (k - w) / n)) / 2
        return lr


def make_scheduler(optimizer, opt):
    """libs/modeling/optim.py:687-717 for ``opt = opt['scheduler']``: {name: 'multistep' | 'cosine' | 'null', itrs_per_epoch,
    warmup_epochs, epochs (cosine), steps and gamma (multistep)}; 'null' gives None"""
    name, per_epoch = opt['name'], int(opt['itrs_per_epoch'])
    if name == 'null':
        return None
    ramp = per_epoch * opt.get('warmup_epochs', 0)                 # epochs -> iterations: the schedulers count step() calls
    if name == 'multistep':
        return LinearWarmupMultiStepLR(optimizer, ramp, [per_epoch * e for e in opt['steps']], gamma=opt.get('gamma', 0.1))
    if name == 'cosine':
        return LinearWarmupCosineAnnealingLR(optimizer, ramp, ramp + per_epoch * opt['epochs'])
    raise NotImplementedError(f"scheduler {name!r} is not implemented ('multistep', 'cosine' and 'null' are)")
