"""One training iteration of the reference's Trainer (libs/worker_v2.py:318-325) as a public call.

``training_forward``: the training-mode forward of PtTransformerEarlyFusionIterative (model.py:567-632) composed from the package's
differentiable pieces, so that ``backward()`` works on what ``loss.PointObjective`` makes of its outputs.
``TrainStep``: zero_grad, forward / objective / backward per micro-batch, the loss-norm update, the gradient norm and clip
coefficient, the fused Adam / AdamW update with the EMA copy (``optim``), scheduler.step().  No host read anywhere in the step.

Dropout: after ``model.enable_dropout()`` the forward applies opt's vid_net / fusion ``proj_pdrop`` and ``path_pdrop`` and the
refinement TCN's rate on the counter-based stream of the library (csrc/dropout.h), one 64-bit key per forward, drawn on the CPU; the
backward recomputes the keep bits from the key (``autograd.DropSpec``).  ``model.enable_dropout(sites='all')`` is the opt-in for the
sites this path alone has (``model._train_dropout_rates()``): ``attn_pdrop`` on the attention maps of the video encoder (local window
or ``mha_win_size = 0``), the fusion's cross attention and the text encoder, drawn inside the attention kernels, forward and backward
(include/decafnet_hip_attn_drop.h); the text encoder's ``proj_pdrop`` / ``path_pdrop`` (group DROP_G_TEXT); the fusion's dropouts again
per pyramid level with ``second_fusion=True`` (group DROP_G_FUSION2, layer ``l * n_layers + i``); and ``vid_net.cdrop`` on the clip
features before ``vid_map``.  The one refusal that remains is ``cdrop`` with the shared front end or a ``scat`` model.

``DataParallelTrainStep``: the same step on every rank of a process group, what the reference gets from wrapping its model in
DistributedDataParallel (worker_v2.py:278-280): parameters broadcast from rank 0, the gradients packed into buckets by a HIP kernel
and all-reduced under the last backward (``dist.GradReducer``), the loss norm summed over the ranks.

The guarded step.  ``TrainStep(..., skip_nonfinite=True)`` keeps one non-finite gradient from destroying the run, without a host read:
the norm's final pass decides on the GPU (include/decafnet_hip_guard.h; a NaN, an inf, or finite elements whose squares overflow fp32
in any tensor, or a non-finite sum reported by a conv-gradient operator), and the update kernel reads the verdict and returns.  On
a skip the parameters, both moments and the EMA copy keep their bits; ``p.grad`` keeps the offending gradient for inspection; the
returned ``grad_norm`` is the non-finite norm and ``last_coef`` is 0.  What a skip does NOT hold back: the loss-norm update (a count
of positive points, always finite), ``scheduler.step()``, ``itr``, and Adam's step count -- the count lives on the host and the
verdict is not read back, so the bias corrections follow ATTEMPTED steps.  ``torch.cuda.amp.GradScaler`` holds the count back; here,
after s skips among t attempts, each correction is 1 - b^t where 1 - b^(t-s) belongs, a factor (1 - b^t) / (1 - b^(t-s)) between
the two, and the step is (1 - b1^(t-s)) / (1 - b1^t) * sqrt((1 - b2^t) / (1 - b2^(t-s))) of what it would be.  For betas
(0.9, 0.999) and one skip that is 0.74 at t = 2, 1.009 at t = 50, 1.0003 at t = 1000 and 1.000007 at t = 5000: negligible past the
warm-up, and nothing accumulates, since the moments themselves are untouched.  With finite gradients the guarded step computes the
bits of the unguarded one.  ``guard.report(names)`` is the one host read (applied, skipped,
the last skipped attempt, the first offending parameter); ``state()`` carries the two counters under 'guard'.

Adam's count on the device.  ``TrainStep(..., device_count=True)`` removes that departure: the optimizer keeps the step count of
every parameter in device memory (``optim.AdamW(device_count=True)``, include/decafnet_hip_clock.h), the update reads it there and a
second tiny kernel advances it -- under the guard only when the step was applied.  After a skip the next update then has the bias
corrections of the count that was actually reached, as with ``GradScaler``.  The option works with or without ``skip_nonfinite``;
on finite batches it computes the bits of the default step.  ``scheduler.step()``, ``itr`` and the loss-norm update still follow
ATTEMPTS, which is what a torch loop with ``GradScaler`` does too (``scaler.step`` may skip the optimizer, the loop still calls
``scheduler.step()``).  ``state()`` / ``load_state()`` need no new key: the counts travel in the optimizer's state dict, in torch's
format, and a checkpoint moves freely between the two settings.

Data.  ``data.TrainLoader`` finds the step's batches: the reference's sampling decisions on the host (``data.VideoCentricTrainData``),
the features in a device-resident ``data.FeatureBank``, a batch assembled by dcf_op_assemble_rows (include/decafnet_hip_batch.h).
``run_epoch(ts, loader, epoch)`` is the loop body of ``Trainer.run`` (worker_v2.py:309-325) on them.

The run.  ``fit(ts, loader, root, ...)`` is ``Trainer.run`` itself: ``run_epoch`` per epoch, ``checkpoint`` where the reference
checkpoints (``models/last.pth``, ``models/{epoch}-{itr}.pth``, ``states/last.pth``) and, every ``eval_run`` epochs or iterations, the
EMA copy evaluated on the validation split -- from a ``data.EvalBank`` with an ``evaluator.DeviceRecallCounter`` (dcf_op_recall_update,
include/decafnet_hip_eval.h) without a host read per video -- and resuming from the two ``last.pth`` files.  ``fit_parallel`` is the same
loop on a process group: rank 0 checkpoints, every rank evaluates its share of the bank and the tables are summed over the ranks, the
validation loss comes from an ``evaluator.DeviceLossMeter`` (dcf_op_loss_table_mean, include/decafnet_hip_fit.h), and
``DataParallelTrainStep(..., agree_skips=True)`` keeps the ranks' skips equal.

The log.  ``fit(..., log_interval=N)`` writes the Trainer's lines to ``<root>/log.txt`` from a ``StepLog``: the loss meters live in
device memory (dcf_op_steplog_add / dcf_op_steplog_flush, include/decafnet_hip_steplog.h), the step adds to them with one launch and
waits for nothing, and a line is written once its numbers have landed.  ``fit(..., data_state=True)`` puts the data loader's random
streams into the checkpoint (``states/data_last.pth``), so that a resumed run with ``crop_ratio`` draws the windows, and logs the
losses, of the uninterrupted one.  Both are off by default.

Not here: W&B and TensorBoard themselves, AMP, graph capture of the step, SGD, gradient compression, the detection
of parameters that no rank used.

The front end.  ``training_forward(..., front_end='dense')`` makes the network's input as the reference does: the features of a video
once per query, transposed, times the gate, concatenated with the shallow features, and ``masked_conv1d`` on that (B', T, Cin)
tensor, which its backward keeps.  ``front_end='shared'`` is ``autograd.gated_vid_map`` (csrc/front_grad.hip,
include/decafnet_hip_front.h): what the inference engine does -- ``W[:, :D] . vid`` and ``W[:, D:2D] . shallow`` once per video, the
64-clip tiles that no query's gate keeps not at all, a row kernel per query -- with a weight gradient on the same shared products, so
nothing of size B' T Cin exists in either direction.  'dense' stays the default (it is what tests/test_gpu_train_step.py pins bit
for bit against ``run_step``).  ``opt.model.scat`` (the raw sidekick score as input channel 2 D + 1) trains through the shared
path alone, whatever ``front_end`` says: the score channel is a rank-1 term there.  ``sfonly`` stays refused (the reference's
training branch, model.py:606-612, never reads it).  ``cdrop`` (with ``enable_dropout(sites='all')``) needs the dense front end and
a model without ``scat``: a per-sample channel mask cannot share products, so the shared path raises ValueError.

The expert features.  ``training_forward(..., expert='selected')`` / ``TrainStep(..., expert='selected', expert_fn=None)`` run ``vid_map``
and its weight gradient on the expert features of the clips the top-k gates keep (``autograd.selected_vid_map``, csrc/front_select.hip,
include/decafnet_hip_front_select.h): after the scores and the gates one compaction launch and ONE host read -- the videos' clip
counts, which a caller with an online expert encoder needs anyway --, then ``expert_fn(b, clips)`` per video or a gather from the dense
batch, then the op on packed (n_rows, D) rows.  No dense expert tensor is read by the op or saved for its backward.  'dense', the
default, launches exactly what it launched before.  At most 16 videos per forward (more: micro-batches); ``cdrop`` and ``sfonly`` are
refused.
"""
import copy
import ctypes
import os
from collections import namedtuple

import torch

from . import _lib, autograd as A, dist as D, loss as L, optim as O


FRONT_ENDS = ('dense', 'shared')
EXPERTS = ('dense', 'selected')
MAX_SELECTED_VIDEOS = 16           # DCF_MAX_VIDEOS of the selected-clip extensions


def _selected_front(model, vid, shallow, vid_masks, gate, mask, correl, sizes, half, expert_fn, selection, vid_rows):
    """The front end of ``training_forward(expert='selected')`` behind the scores and the gates: the selection (one launch and ONE host
    read, of the videos' counts), the packed expert rows, and ``autograd.selected_vid_map`` -> (vid_map (B', T, E), mask (B', T) bool)"""
    from . import modeling
    bs, D, T = shallow.shape
    dev = shallow.device
    if selection is None:                                           # dcf_op_select_clips_videos on the gates dcf_op_gate just wrote
        vm = vid_masks.reshape(bs, T).to(torch.bool).contiguous()
        lists = torch.empty(2 * bs * T + bs, device=dev, dtype=torch.int32)           # clips, pos and counts: one allocation
        clips, pos, counts = lists[:bs * T].view(bs, T), lists[bs * T:2 * bs * T].view(bs, T), lists[2 * bs * T:]
        nqs = torch.tensor(sizes, dtype=torch.int32)
        _lib.check(_lib.lib().dcf_op_select_clips_videos(_lib.ptr(gate), _lib.ptr(vm), T, bs, ctypes.cast(nqs.data_ptr(), _lib._IP),
                                                         _lib.ptr(clips), _lib.ptr(pos), _lib.ptr(counts), _lib.current_stream()),
                   'dcf_op_select_clips_videos')
        selection = modeling.SelectionBatch(gate, pos, clips, correl if model.scat else None, counts.cpu().tolist(), sizes)
    else:                                                           # the caller's: its gate decides, the mask follows it as dcf_op_gate defines it
        if selection.nvid != bs or list(selection.nqs) != list(sizes) or selection.T != T:
            raise ValueError(f'training_forward: the selection is for {selection.nvid} videos with {selection.nqs} queries on '
                             f'{selection.T} clips, the batch has {bs} videos with {list(sizes)} on {T}')
        if model.scat and selection.scores is None:
            raise ValueError('training_forward: opt.model.scat needs the sidekick scores: the selection carries none')
        gate = selection.gate.float().contiguous()
        mask = vid_masks.reshape(bs, T).to(torch.bool).repeat_interleave(torch.tensor(sizes, device=dev), dim=0)
        if not model.msf:
            mask = mask & (gate != 0)
    if min(selection.counts) < 1:
        raise ValueError(f'training_forward: a video of the selection is empty (counts {selection.counts}): no clip of it is valid')
    if vid_rows is not None:
        rows = vid_rows
    elif expert_fn is not None:                                     # once per video, on the host's ascending clip list, packed
        rows = torch.cat([expert_fn(b, selection.clips_host(b)) for b in range(bs)])
    else:
        rows = model.gather_clip_rows_videos([vid[b:b + 1] for b in range(bs)], selection)
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dim() == 2 and rows.size(1) == D and rows.size(0) >= selection.n_rows):
        raise ValueError(f'training_forward: the expert rows are {tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__}, the '
                         f'selection needs ({selection.n_rows}, {D}) on the GPU: one row of D expert features per selected clip')
    if half and rows.dtype != torch.float16:
        modeling._check_feature_dtypes(rows, shallow)
    if not half:
        rows = rows.float()
    model.last_train_feature_dtype = torch.float16 if half else torch.float32
    y = A.selected_vid_map(rows, selection.row_first, selection.pos, shallow if model.msf else None, gate, mask,
                           selection.scores if model.scat else None, sizes, model.vid_map.conv.weight, model.vid_map.conv.bias)
    return y, mask


def training_forward(model, vid, shallow, vid_masks, tokens, text_cls, token_masks, text_size=None, dropout=None, dropout_seed=None,
                     front_end='dense', expert='dense', expert_fn=None, selection=None, vid_rows=None):
    """vid / shallow (bs, D, T) channel-major, vid_masks (bs, T) bool, tokens (B', C_t, Lq) channel-major, text_cls (B', D),
    token_masks (B', 1, Lq) or (B', Lq), text_size: queries per video (None: one each), B' = sum(text_size), all on the GPU.
    -> (fpn_logits1, fpn_logits2, fpn_offsets, fpn_masks) as ``model(..., eval=False)`` returns them, with an autograd graph to every
    parameter of the model.  Per video the sidekick scores and the block top-k gate (dcf_op_sidekick / dcf_op_gate, not
    differentiated: the gate is a 0 / 1 weight), the product and the concatenation with the shallow features, vid_map, the text
    encoder, the first fusion, the video encoder, then the heads with the refinement stage (``autograd.fuse_and_predict``).
    ``dropout``: the (seed, p, b0) of ``autograd.fuse_and_predict`` for the refinement stage's dropout alone, None for none; only
    for a model without ``enable_dropout()``.  With ``model.enable_dropout()`` the forward applies the rates of
    ``model._train_dropout_rates()`` (the five of ``model._dropout_rates()``; with ``sites='all'`` every rate of opt) with b0 = 0 under one 64-bit key: ``dropout_seed`` if given, else ``model._next_dropout_seed()``
    (the CPU generator ``enable_dropout`` set up); the key is left in ``model.last_dropout_seed``.
    ``vid`` / ``shallow`` may be float16, both or neither.  With ``front_end='shared'`` (or a ``scat`` model) and
    ``model.half_features`` (default True) a float16 pair is read as it is stored -- dcf_op_sidekick_h for the scores,
    ``autograd.gated_vid_map`` on the float16 tensors, which its backward keeps: no fp32 copy of the features exists -- and every output
    and gradient has the bits of the same values passed as fp32.  ``model.last_train_feature_dtype`` says what ``gated_vid_map`` was
    handed (torch.float16 or torch.float32); the dense front end and ``half_features = False`` upcast as before.
    ``front_end``: how the input of the network is made of the features.  'dense' builds the reference's (B', T, Cin) tensor --
    every video's features once per query, gated, concatenated -- and runs ``masked_conv1d`` on it.  'shared' is
    ``autograd.gated_vid_map``: the products of ``vid_map`` with the features once per video, clips that no query's gate keeps not at
    all, no (B', T, Cin) tensor in the forward or saved for the backward.  A model with ``opt.model.scat`` always takes the shared
    path (its 2 D + 1 input channels do not fit the dense weight gradient), with the scores dcf_op_sidekick returns.
    ``expert``: 'dense' reads the expert features ``vid`` of every clip and launches exactly what it launched before the option
    existed.  'selected' runs vid_map on the expert features of the clips the gates keep (``autograd.selected_vid_map``,
    include/decafnet_hip_front_select.h), whatever ``front_end`` says, ``scat`` included: first the selection (the scores and the
    gates as on every path, then dcf_op_select_clips_videos on them -- the compaction ``model.select_clips_videos`` ends with -- and
    ONE host read, of the videos' counts; the engine is not bound and ``vid_net.stride`` does not matter: vid_map sees the input clips), then the rows --
    ``vid_rows`` (packed, with the ``selection`` they were made for) if given, else ``expert_fn(b, clips)`` once per video b with its
    ascending clip list as a CPU int64 tensor, returning (len(clips), D) on the GPU (``vid`` may then be None), else gathered from the
    dense ``vid`` (``model.gather_clip_rows_videos``: the emulation path) -- then the op.  Nothing of size (bs, D, T) is read or saved
    on the expert side.  ``shallow`` alone decides the feature type (a float16 ``shallow`` with ``model.half_features`` takes float16
    rows).  At most 16 videos per forward; ``sfonly`` and ``cdrop`` are refused."""
    from . import modeling
    if front_end not in FRONT_ENDS:
        raise ValueError(f'training_forward: front_end = {front_end!r} (one of {FRONT_ENDS})')
    if expert not in EXPERTS:
        raise ValueError(f'training_forward: expert = {expert!r} (one of {EXPERTS})')
    selected = expert == 'selected'
    if not selected and (expert_fn is not None or selection is not None or vid_rows is not None):
        raise ValueError("training_forward: expert_fn / selection / vid_rows belong to expert='selected'")
    if (vid_rows is None) != (selection is None):
        raise ValueError('training_forward: vid_rows and selection come together (the packed rows and the selection they were made for)')
    if type(model) is not modeling.PtTransformerEarlyFusionIterative:
        raise NotImplementedError(f'training_forward: {type(model).__name__} is not implemented (PtTransformerEarlyFusionIterative only)')
    if model.sfonly:
        raise NotImplementedError('training_forward: opt.model.sfonly is not implemented: the training branch of the reference '
                                  '(model.py:606-612) never reads it')
    shared = front_end == 'shared' or bool(model.scat) or selected
    rates = model._train_dropout_rates()                            # None without enable_dropout(); refuses what has no kernel
    if rates is not None and rates.cdrop > 0.0 and selected:
        raise ValueError("training_forward: opt.model.vid_net.cdrop > 0 needs expert='dense' with front_end='dense': a per-sample "
                         "channel mask cannot share the expert product between the queries of a video")
    if rates is not None and rates.cdrop > 0.0 and shared:
        raise ValueError("training_forward: opt.model.vid_net.cdrop > 0 needs front_end='dense' on a model without scat: a per-sample "
                         "channel mask cannot share the products of vid_map between the queries of a video")
    if rates is None and dropout_seed is not None:
        raise ValueError('training_forward: dropout_seed without model.enable_dropout()')
    if rates is not None and dropout is not None:
        raise ValueError('training_forward: `dropout` is the refinement stage alone on a model without enable_dropout(); this model\'s '
                         'dropout is enabled and covers it')
    if selected:
        if shallow.size(0) > MAX_SELECTED_VIDEOS:
            raise ValueError(f"training_forward: expert='selected' takes at most {MAX_SELECTED_VIDEOS} videos per forward (got "
                             f'{shallow.size(0)}): split the step into micro-batches (TrainStep.step takes a list of them)')
        if vid is None and expert_fn is None and vid_rows is None:
            raise ValueError("training_forward: expert='selected' without `vid` needs expert_fn or vid_rows")
    if not (shallow if selected else vid).is_cuda:
        raise RuntimeError('the training forward runs on the MI355X only: move the inputs to the GPU')
    lib, st = _lib.lib(), _lib.current_stream()
    bs, D, T = shallow.shape if selected else vid.shape
    sizes = [1] * bs if text_size is None else [int(k) for k in text_size]
    nq = sum(sizes)
    if len(sizes) != bs or min(sizes) < 1 or tokens.size(0) != nq or text_cls.size(0) != nq:
        raise ValueError(f'text_size {sizes} does not match {bs} videos, {tokens.size(0)} token rows and {text_cls.size(0)} text_cls rows')
    # float16 features go to the sidekick scores and to gated_vid_map as they are stored (include/decafnet_hip_half.h,
    # include/decafnet_hip_front_half.h); the dense front end builds an fp32 (B', T, Cin) tensor anyway and keeps its upcast
    half = False
    if shared and model.half_features:
        if vid is not None:
            modeling._check_feature_dtypes(vid, shallow)
        half = shallow.dtype == torch.float16
    model.last_train_feature_dtype = torch.float16 if half else torch.float32
    if shared and not half:
        vid, shallow = (None if vid is None else vid.float()), shallow.float()
    gates, masks, correls, q = [], [], [], 0
    for b, k in enumerate(sizes):                                   # one video and its k queries per call
        sh, cls = (shallow[b] if half else shallow[b].float()).contiguous(), text_cls[q:q + k].float().contiguous()
        vm = vid_masks[b].reshape(-1).to(torch.bool).contiguous()
        correl = torch.empty(k, T, device=shallow.device)
        sidekick = 'dcf_op_sidekick_h' if half else 'dcf_op_sidekick'
        _lib.check(getattr(lib, sidekick)(_lib.ptr(sh), _lib.ptr(cls), _lib.ptr(correl), D, T, k, int(model.norm), st), sidekick)
        gate, mo = torch.empty(k, T, device=shallow.device), torch.empty(k, T, dtype=torch.bool, device=shallow.device)
        _lib.check(lib.dcf_op_gate(_lib.ptr(correl), _lib.ptr(vm), _lib.ptr(gate), _lib.ptr(mo), T, k, model.sn, float(model.sratio),
                                   int(model.msf), st), 'dcf_op_gate')
        gates.append(gate), masks.append(mo), correls.append(correl)
        q += k
    gate, mask = torch.cat(gates), torch.cat(masks)
    kv_size = torch.tensor(sizes, device=shallow.device)
    vid_drop = fus_drop = text_drop = None
    if rates is not None:                                           # one key per forward
        seed = (model._next_dropout_seed() if dropout_seed is None else int(dropout_seed)) & ((1 << 64) - 1)
        model.last_dropout_seed = seed
        vid_drop = A.DropSpec(seed, 0, rates.vid_net.proj, rates.vid_net.path, attn_p=rates.vid_net.attn)
        fus_drop = A.DropSpec(seed, 0, rates.fusion.proj, rates.fusion.path, attn_p=rates.fusion.attn)
        text_drop = A.DropSpec(seed, 0, rates.text_net.proj, rates.text_net.path, attn_p=rates.text_net.attn)
        if rates.refine > 0.0:
            dropout = (seed, rates.refine, 0)
    if selected:                                                    # the expert half on the rows of the selected clips alone
        vid_map, mask = _selected_front(model, vid, shallow.contiguous(), vid_masks, gate, mask, torch.cat(correls), sizes, half, expert_fn,
                                        selection, vid_rows)
    elif shared:                                                    # the products once per video: nothing is repeated or transposed
        vid_map = A.gated_vid_map(vid, shallow if model.msf else None, gate, mask, torch.cat(correls) if model.scat else None, sizes,
                                  model.vid_map.conv.weight, model.vid_map.conv.bias)
    else:
        rep = lambda z: z.transpose(1, 2).contiguous().repeat_interleave(kv_size, dim=0)     # model.py:578-581: video b once per query
        x = rep(vid) * gate[..., None]
        if model.msf:
            x = torch.cat([x, rep(shallow)], dim=2)
        if rates is not None and rates.cdrop > 0.0:                 # model.py:614: nn.Dropout1d on the (B', Cin, T) tensor
            x = A.channel_dropout(x, A.DropSpec(seed, 0, proj_p=rates.cdrop, group=A.DROP_G_INPUT))
        vid_map = A.masked_conv1d(x, mask, model.vid_map.conv.weight, model.vid_map.conv.bias)
    text, text_mask = A.text_transformer(tokens.transpose(1, 2).contiguous(), token_masks.reshape(nq, -1), model.text_net,
                                         **({} if text_drop is None or not text_drop.active else {'drop': text_drop}))
    fused, fmask = A.xattn_fusion(vid_map, mask, text, text_mask, model.fusion, kv_size, **({} if fus_drop is None else {'drop': fus_drop}))
    fpn, fpn_masks = A.video_transformer(fused, fmask, model.vid_net, **({} if vid_drop is None else {'drop': vid_drop}))
    extra = dict(text=text, text_mask=text_mask, kv_size=kv_size) if model.second_fusion else {}
    if model.second_fusion and fus_drop is not None and fus_drop.active:
        extra['fusion_drop'] = fus_drop
    if dropout is not None:
        extra['dropout'] = dropout
    return A.fuse_and_predict(fpn, fpn_masks, model, **extra)


_BATCH_KEYS = ('vid', 'shallow', 'vid_masks', 'tokens', 'text_cls', 'token_masks', 'text_size')


class TrainStep:
    """What the Trainer owns for its iteration: the objective, the optimizer (``optim.make_optimizer``), the scheduler
    (``optim.make_scheduler``), the EMA copy and the ``itr`` counter.  ``opt`` is the ``config.make_opt`` tree; ``itrs_per_epoch``
    is what the Trainer takes from its data loader (worker_v2.py:252).  The model is on the GPU.  ``front_end``: 'dense' or 'shared',
    handed to ``training_forward`` (a ``scat`` model takes the shared path either way).  ``skip_nonfinite=True``: the step owns an
    ``optim.StepGuard`` (``self.guard``), armed around forward, backward and update; a step whose gradients are not all finite is
    skipped on the GPU (module docstring).  ``False`` -- the default -- launches exactly what it launched before the option existed.
    ``device_count=True``: Adam's step counts live on the GPU and advance on applied steps only (module docstring); the scheduler,
    ``itr`` and the loss-norm update still follow attempts.  ``False`` -- the default -- changes nothing.
    ``expert``: 'dense' or 'selected', and ``expert_fn``, handed to ``training_forward``: with 'selected' vid_map runs on the expert
    features of the clips the gates keep -- from ``expert_fn(b, clips)`` per video of a micro-batch if given (the batch's 'vid' may then
    be None), else gathered from the batch's dense 'vid', which is what ``fit`` on a ``data.TrainLoader`` does.  'dense' -- the default
    -- launches exactly what it launched before the option existed.  Like ``front_end`` it is a property of the step, not of the
    checkpoint: ``state()`` / ``load_state()`` carry neither, and a checkpoint moves freely between the settings."""

    def __init__(self, model, opt, world_size=1, itrs_per_epoch=1, front_end='dense', skip_nonfinite=False, device_count=False,
                 expert='dense', expert_fn=None):
        if front_end not in FRONT_ENDS:
            raise ValueError(f'TrainStep: front_end = {front_end!r} (one of {FRONT_ENDS})')
        if expert not in EXPERTS:
            raise ValueError(f'TrainStep: expert = {expert!r} (one of {EXPERTS})')
        if expert_fn is not None and expert != 'selected':
            raise ValueError("TrainStep: expert_fn belongs to expert='selected'")
        self.expert, self.expert_fn = expert, expert_fn
        if not isinstance(skip_nonfinite, bool):
            raise ValueError(f'TrainStep: skip_nonfinite = {skip_nonfinite!r} (True or False)')
        if not isinstance(device_count, bool):
            raise ValueError(f'TrainStep: device_count = {device_count!r} (True or False)')
        self.model, self.opt, self.front_end, self.skip_nonfinite = model, opt, front_end, skip_nonfinite
        self.device_count = device_count
        self.objective = L.PointObjective(opt, world_size=world_size)
        self.optimizer = O.make_optimizer(model, opt['optimizer'], device_count=device_count)
        sched = copy.deepcopy(dict(opt['scheduler']))                       # opt.py:467-468, worker_v2.py:252, on a copy
        sched.update({k: opt['train'][k] for k in ('epochs', 'warmup_epochs') if k in opt['train']}, itrs_per_epoch=int(itrs_per_epoch))
        self.scheduler = O.make_scheduler(self.optimizer, sched)
        self.clip_grad_norm = opt['optimizer']['clip_grad_norm']
        self.ema = O.ModelEma(model, opt['train'].get('ema_beta', 0.999)).attach(self.optimizer)
        self.epoch = self.itr = 0
        self.last_coef = None                                               # the clip coefficient of the last step (a device tensor)
        self._norm_table = O._Table()
        self._params = list(model.parameters())
        self.guard, self._guard_counters = None, (0, 0)                     # the StepGuard of skip_nonfinite, made once the model is on the GPU
        self._ensure_guard()

    def _ensure_guard(self):
        """the step guard of ``skip_nonfinite=True``, or None: without the option, and while the model is not on the GPU (the forward
        refuses that below, as it does without the option)"""
        if self.guard is None and self.skip_nonfinite and self._params and self._params[0].is_cuda:
            self.guard = O.StepGuard(self._params[0].device).load_counters(*self._guard_counters)
        return self.guard

    def step(self, batch, targets):
        """``batch``: a dict with the arguments of ``training_forward`` (vid, shallow, vid_masks, tokens, text_cls, token_masks,
        text_size), or a list of such dicts, one per micro-batch, with ``targets`` (B', 2) a tensor or a list alike.  The gradients of
        the micro-batches accumulate before the one update (worker_v2.py:366-376).
        -> {'cls', 'reg', 'total', 'grad_norm'}: device tensors, summed over the micro-batches.  ``p.grad`` keeps the UNCLIPPED
        gradient: the clip coefficient is folded into the update."""
        batches, targets = ([batch], [targets]) if isinstance(batch, dict) else (list(batch), list(targets))
        if len(batches) != len(targets) or not batches:
            raise ValueError(f'{len(batches)} micro-batches and {len(targets)} target tensors')
        guard = self._ensure_guard()
        if guard is None:
            return self._step(batches, targets, None)
        guard.arm()                                        # a non-finite sum in a conv gradient becomes a skip, not a failed next call
        try:
            return self._step(batches, targets, guard)
        finally:
            guard.disarm()

    def _step(self, batches, targets, guard):
        self.optimizer.zero_grad(set_to_none=True)
        sums = {}
        for i, (mb, tg) in enumerate(zip(batches, targets)):
            extra = {} if self.expert == 'dense' else {'expert': self.expert, 'expert_fn': self.expert_fn}
            out = training_forward(self.model, *(mb.get(k) for k in _BATCH_KEYS), front_end=self.front_end, **extra)
            d = self.objective(out, tg)
            self._backward(d['total'], i == len(batches) - 1)
            for k, v in d.items():
                sums[k] = v.detach() if k not in sums else sums[k] + v.detach()
        self.objective.update_norm(self._norm_over_ranks(sums.pop('norm')))
        norm, coef = O.grad_norm_and_coef(self._params, self.clip_grad_norm or 0.0, _table=self._norm_table, guard=guard)
        self.last_coef = coef if self.clip_grad_norm else None
        self.optimizer.step(clip_coef=self.last_coef, guard=guard)
        if self.scheduler is not None:
            self.scheduler.step()
        self.itr += 1
        sums['grad_norm'] = norm
        return sums

    def _backward(self, total, last):
        """the backward of one micro-batch; ``last``: no further one follows before the update"""
        total.backward()

    def _norm_over_ranks(self, norm):
        """the step's norm summed over the ranks (worker_v2.py:379-380): one rank here"""
        return norm

    def state(self):
        """-> (model_ckpt, state_ckpt) with the keys of Trainer.checkpoint (worker_v2.py:680-689).  'loss_norm' is an addition
        (the reference does not save its running normaliser) and costs a host read, like the checkpoint itself.  'dropout_rng' is
        another, present only when ``model.enable_dropout`` was given an int seed: the state of the private generator that hands out
        the dropout keys, so that a resumed run draws the keys the uninterrupted one would."""
        snap = copy.deepcopy                                               # a snapshot: state_dict() hands out the live tensors
        state = {'optimizer': snap(self.optimizer.state_dict()),
                 'scheduler': None if self.scheduler is None else snap(self.scheduler.state_dict()),
                 'epoch': self.epoch, 'itr': self.itr, 'loss_norm': self.objective.loss_norm}
        gen = self._dropout_generator()
        if gen is not None:
            state['dropout_rng'] = gen.get_state().clone()
        if self.skip_nonfinite:                                            # the guard's two counters: a host read, like the rest
            rep = None if self.guard is None else self.guard.report()
            a, k = self._guard_counters if rep is None else (rep['applied'], rep['skipped'])
            state['guard'] = {'applied': a, 'skipped': k}
        return {'model': snap(self.model.state_dict()), 'model_ema': snap(self.ema.state_dict())}, state

    def _dropout_generator(self):
        """the private CPU generator of ``model.enable_dropout(seed=<int>)``, or None"""
        d = getattr(self.model, '_dropout', None)
        return None if d is None else d[1]

    def load_state(self, model_ckpt, state_ckpt):
        self.model.load_state_dict(model_ckpt['model'])
        self.ema.load_state_dict(model_ckpt['model_ema'])
        self.optimizer.load_state_dict(state_ckpt['optimizer'])
        if self.scheduler is not None:
            self.scheduler.load_state_dict(state_ckpt['scheduler'])
        self.epoch, self.itr = state_ckpt['epoch'], state_ckpt['itr']
        if 'loss_norm' in state_ckpt:
            self.objective.loss_norm = state_ckpt['loss_norm']
        if 'dropout_rng' in state_ckpt:
            gen = self._dropout_generator()
            if gen is None:
                raise ValueError('load_state: the checkpoint carries a dropout generator state; call model.enable_dropout(seed=<int>) first')
            gen.set_state(state_ckpt['dropout_rng'])
        if self.skip_nonfinite and 'guard' in state_ckpt:
            self._guard_counters = (int(state_ckpt['guard']['applied']), int(state_ckpt['guard']['skipped']))
            if self._ensure_guard() is not None:
                self.guard.load_counters(*self._guard_counters)
        return self


def run_epoch(ts, loader, epoch=None, log=None):
    """One epoch of ``Trainer.run`` (worker_v2.py:309-325) without its evaluation: ``ts.step`` on every batch of
    ``loader.epoch(epoch)`` (a ``data.TrainLoader``; ``epoch`` None: ``ts.epoch``), then ``ts.epoch = epoch + 1``.  ``log``: a
    ``StepLog`` that is updated after every step (None, the default: nothing more is launched).
    -> the running sums of what the steps returned (cls, reg, total, grad_norm) as device tensors, and 'steps', an int.  No host read."""
    epoch = ts.epoch if epoch is None else int(epoch)
    sums, steps = {}, 0
    for batch, targets in loader.epoch(epoch):
        out = ts.step(batch, targets)
        if log is not None:
            log.update(out)
        for k, v in out.items():
            sums[k] = v if k not in sums else sums[k] + v
        steps += 1
    ts.epoch = epoch + 1
    sums['steps'] = steps
    return sums


STEP_KEYS = ('cls', 'reg', 'total', 'grad_norm')                     # what ``TrainStep.step`` returns
LOG_STATS = ('mean', 'finite_mean', 'min', 'max', 'last', 'n_finite')  # the columns of a row of dcf_op_steplog_flush


def time_str(t):
    """libs/train_utils.py:56-61"""
    if t >= 3600:
        return '{:.1f}h'.format(t / 3600)
    if t > 60:
        return '{:.1f}m'.format(t / 60)
    return '{:.1f}s'.format(t)


def log_line(itr, num_itrs, keys, means, seconds):
    """the line of ``Trainer.log`` (worker_v2.py:705-720): the iteration in the width of ``num_itrs``, ``key mean | `` per key in the
    order of ``keys``, then ``time_str`` of the seconds per step"""
    t = len(str(num_itrs))
    return f'[{itr:0{t}d}/{num_itrs:0{t}d}] ' + ''.join(f'{k} {m:.3f} | ' for k, m in zip(keys, means)) + time_str(seconds)


def _log_arguments(who, log_interval, log_keys):
    """the checks ``StepLog``, ``fit`` and ``fit_parallel`` share -> (log_interval as an int, the keys as a tuple)"""
    if isinstance(log_interval, bool) or int(log_interval) != log_interval or int(log_interval) < 0:
        raise ValueError(f'{who}: log_interval = {log_interval!r} (an int >= 0; 0: no log)')
    keys = (log_keys,) if isinstance(log_keys, str) else tuple(log_keys)
    bad = [k for k in keys if k not in STEP_KEYS]
    if bad or not keys or len(set(keys)) != len(keys) or len(keys) > _lib.STEPLOG_MAX_KEYS:
        raise ValueError(f'{who}: log_keys = {log_keys!r}: a non-empty selection without repeats of what the step returns, {STEP_KEYS}')
    return int(log_interval), keys


class StepLog:
    """The Trainer's loss meters and log lines (worker_v2.py:326-335, 705-720) without a host wait in the loop.

    The reference calls ``v.detach().item()`` on every loss of every step: a wait per step, which ``TrainStep.step`` is built to avoid.
    Here the meters are two small tables in device memory (include/decafnet_hip_steplog.h).  ``update(step_out)``, called after
    ``ts.step`` on the stream the step ran on, adds the step's values with ONE launch (dcf_op_steplog_add gathers the ``keys`` from
    their separate allocations).  When ``ts.itr == 1 or ts.itr % log_interval == 0`` (worker_v2.py:334) it also makes one
    dcf_op_steplog_flush (read-and-reset, in stream order), one ``non_blocking`` copy of the (K + 1, 6) result into a pinned buffer and
    one timing event, queues ``(itr, buffer, event)`` and goes on.  ``poll()`` -- every ``update`` ends with one -- writes the lines of
    all entries at the head of the queue whose event has completed, in order, and never waits; ``drain()`` waits for the last event
    and writes everything; ``close()`` drains.

    The line is the reference's: ``[{itr}/{num_itrs}] `` in the width of ``num_itrs``, ``{key} {mean:.3f} | `` per key in ``keys``
    order (any selection of cls, reg, total, grad_norm), then ``time_str`` of the seconds per step.  The mean is AverageMeter's:
    ``sum / steps`` with the sum taken in step order in double, the bits of ``sum += float(v)``.  Seconds per step is DEVICE time: the
    time between this flush's event and the previous one's (for the first line: the event recorded at construction) over the
    interval's steps.  The reference's host clock around a step would measure enqueueing here.

    The line is appended to ``path`` (None: no file; the loops pass ``<root>/log.txt``, worker_v2.py:263), so a resumed run continues
    the file; it is printed with ``echo=True``; and ``on_line(itr, {key: {'mean', 'finite_mean', 'min', 'max', 'last', 'n_finite'}},
    steps, seconds)`` is where a W&B or TensorBoard user attaches (neither is imported here).  ``finite_mean`` / ``min`` / ``max``
    cover the finite values alone (NaN where there is none): what a run under ``skip_nonfinite`` wants to see beside a mean that one
    NaN poisons, as in the reference.

    A partial interval is not part of a checkpoint: a resumed run starts its meters empty."""

    def __init__(self, ts, num_itrs, path=None, log_interval=100, keys=('cls', 'reg', 'total'), echo=False, on_line=None):
        log_interval, self.keys = _log_arguments('StepLog', log_interval, keys)
        if log_interval < 1:
            raise ValueError(f'StepLog: log_interval = {log_interval!r} (>= 1)')
        if on_line is not None and not callable(on_line):
            raise ValueError(f'StepLog: on_line = {on_line!r} is not callable')
        self.ts, self.num_itrs, self.path, self.log_interval, self.echo, self.on_line = ts, int(num_itrs), path, log_interval, echo, on_line
        self.device = ts._params[0].device
        if self.device.type != 'cuda':
            raise RuntimeError('StepLog: the meters live on the MI355X: move the model to the GPU first')
        K = len(self.keys)
        self._lib = _lib.lib()
        self._stats = torch.zeros(K, _lib.STEPLOG_COLS, dtype=torch.float64, device=self.device)
        self._counts = torch.zeros(K + 1, dtype=torch.int64, device=self.device)
        self._out = torch.empty(K + 1, _lib.STEPLOG_COLS, dtype=torch.float64, device=self.device)
        self._free = [self._pinned() for _ in range(2)]
        self._pending = []                                                # (itr, pinned buffer, event), oldest first
        self._vals = (_lib.vp * K)()
        self._last_event = torch.cuda.Event(enable_timing=True)
        self._last_event.record()
        self.lines = 0                                                     # lines written so far

    def _pinned(self):
        return torch.empty(len(self.keys) + 1, _lib.STEPLOG_COLS, dtype=torch.float64).pin_memory()

    def update(self, step_out):
        """the values of one step (what ``ts.step`` returned) into the meters; a flush where the reference logs; then ``poll()``"""
        st, K = _lib.current_stream(), len(self.keys)
        for i, k in enumerate(self.keys):
            v = step_out[k]
            if v.dtype != torch.float32 or v.numel() != 1 or v.device != self.device:
                raise ValueError(f'StepLog.update: {k!r} is {v.dtype} of {tuple(v.shape)} on {v.device}: one fp32 scalar on {self.device}')
            self._vals[i] = v.data_ptr()
        _lib.check(self._lib.dcf_op_steplog_add(self._vals, K, _lib.ptr(self._stats), _lib.ptr(self._counts), st), 'dcf_op_steplog_add')
        itr = self.ts.itr
        if itr == 1 or itr % self.log_interval == 0:                       # worker_v2.py:334
            _lib.check(self._lib.dcf_op_steplog_flush(_lib.ptr(self._stats), _lib.ptr(self._counts), K, _lib.ptr(self._out), st),
                       'dcf_op_steplog_flush')
            buf = self._free.pop() if self._free else self._pinned()
            buf.copy_(self._out, non_blocking=True)                        # stream order: before the next flush rewrites ``_out``
            event = torch.cuda.Event(enable_timing=True)
            event.record()
            self._pending.append((itr, buf, event))
        self.poll()

    def poll(self):
        """write the lines whose numbers have landed, oldest first; never waits -> how many were written"""
        n = 0
        while self._pending and self._pending[0][2].query():
            self._write(*self._pending.pop(0))
            n += 1
        return n

    def drain(self):
        """wait for the last pending flush and write every line -> how many were written"""
        if self._pending:
            self._pending[-1][2].synchronize()
        return self.poll()

    close = drain

    def _write(self, itr, buf, event):
        rows = buf.tolist()
        self._free.append(buf)
        steps = int(rows[-1][0])
        seconds = self._last_event.elapsed_time(event) * 1e-3 / max(steps, 1)
        self._last_event = event
        line = log_line(itr, self.num_itrs, self.keys, [r[0] for r in rows[:-1]], seconds)
        if self.path is not None:
            with open(self.path, 'a') as fh:
                fh.write(line + '\n')
        if self.echo:
            print(line, flush=True)
        self.lines += 1
        if self.on_line is not None:
            self.on_line(itr, {k: dict(zip(LOG_STATS, r)) for k, r in zip(self.keys, rows)}, steps, seconds)


EVAL_BY = ('epoch', 'itr')


def checkpoint(ts, root):
    """Trainer.checkpoint (worker_v2.py:675-692) from ``ts.state()``: ``<root>/models/last.pth`` and ``models/{epoch}-{itr}.pth``
    ({'model', 'model_ema'}) and ``<root>/states/last.pth`` ({'optimizer', 'scheduler', 'epoch', 'itr'} plus the additions
    ``TrainStep.state`` documents).  -> the three paths.  The layout ``GroundingEvaluator.from_checkpoint`` reads."""
    model_ckpt, state_ckpt = ts.state()
    model_dir, state_dir = os.path.join(root, 'models'), os.path.join(root, 'states')
    os.makedirs(model_dir, exist_ok=True)
    os.makedirs(state_dir, exist_ok=True)
    paths = (os.path.join(model_dir, 'last.pth'), os.path.join(model_dir, f'{ts.epoch}-{ts.itr}.pth'), os.path.join(state_dir, 'last.pth'))
    torch.save(model_ckpt, paths[0])
    torch.save(model_ckpt, paths[1])
    torch.save(state_ckpt, paths[2])
    return paths


def evaluate(ts, evaluator, eval_data, counter=None, meter=None):
    """The EMA copy (``ts.ema.module``: its own module, in eval mode, with an engine of its own) through ``evaluator`` on ``eval_data``
    -> the counter.  A ``data.EvalBank`` (or a ``subset`` of one) without a counter gets an ``evaluator.DeviceRecallCounter``: the pass
    then reads nothing back before the counter's accessors.  ``meter``: an ``evaluator.DeviceLossMeter`` of that bank, filled beside
    the counter (``GroundingEvaluator.run(loss_meter=)``).  The training model, its mode, its dropout generator and its engines are
    not touched; the evaluator's own model is put back afterwards."""
    from . import data as _data, evaluator as E
    opt_eval = ts.opt['eval']
    if counter is None:
        ranks, threshs = opt_eval.get('ranks', (1, 5)), opt_eval.get('iou_threshs', (0.3, 0.5))
        dev = next(ts.ema.module.parameters()).device
        banked = isinstance(eval_data, (_data.EvalBank, _data.EvalBankSubset))
        counter = E.DeviceRecallCounter(ranks, threshs, dev) if banked else E.RecallCounter(ranks, threshs)
    ev = evaluator if evaluator is not None else E.GroundingEvaluator(ts.opt, ts.ema.module)
    own, ev.model = ev.model, ts.ema.module
    try:
        return ev.run(eval_data, counter=counter) if meter is None else ev.run(eval_data, counter=counter, loss_meter=meter)
    finally:
        ev.model = own


def fit(ts, loader, root, num_epochs=None, evaluator=None, eval_data=None, eval_by='epoch', eval_run=0, resume=True, log_interval=0,
        log_keys=('cls', 'reg', 'total'), on_line=None, data_state=False):
    """``Trainer.run`` (worker_v2.py:307-364) with its checkpoints, evaluations and log: ``run_epoch`` per epoch until
    ``ts.epoch`` reaches ``num_epochs`` (None: ``opt.train.epochs``).  Where the reference calls ``evaluate(ct)`` -- after every epoch
    with ``eval_by='epoch'`` (ct = the epoch count), after every iteration divisible by ``eval_run`` with ``eval_by='itr'`` (the step
    loop is written out for it; ct = ``ts.itr``) -- ``checkpoint(ts, root)`` runs, and when ``eval_run > 0`` and ct is divisible by it
    the EMA copy is evaluated on ``eval_data`` (``evaluate`` above) and ``counter.report()`` goes to ``<root>/eval_{epoch}_{itr}.txt``.
    ``eval_run=0``: checkpoints per epoch, no evaluation (``eval_by='itr'`` then never checkpoints: the reference divides by it).
    ``resume=True``: when ``models/last.pth`` and ``states/last.pth`` both exist they are loaded first (train.py:66-69) and the loop
    continues at ``ts.epoch``; a checkpoint taken inside an epoch restarts that epoch, as in the reference.
    -> [(epoch, itr, metrics)] of the evaluations.
    ``log_interval > 0``: the Trainer's log.  A ``StepLog`` with ``num_itrs = num_epochs * len(loader)``, ``path = <root>/log.txt``,
    ``keys = log_keys`` and ``on_line`` is updated after every step -- one small launch per step, one more and a 192-byte asynchronous
    copy per logged iteration, no host wait -- and drained before every checkpoint (which reads the device anyway) and before the
    return.  ``log_interval=0``, the default: nothing of it is constructed, launched or written.  A negative interval and a key the
    step does not return are refused with ValueError before anything is opened.
    ``data_state=True``: the data loader's random streams become part of a checkpoint.  ``checkpoint`` is followed by
    ``<root>/states/data_last.pth`` (``loader.state()``: inside an epoch the streams as they were at its start, since a resumed run
    restarts that epoch), and a resume loads the file where it exists, so that with ``crop_ratio`` set the resumed run draws the
    windows of the uninterrupted one.  ``False``, the default: the files under ``root`` are what they were, and the streams start over.
    Not here: the validation loss, W&B itself, more than one rank (NotImplementedError before anything is launched; ``fit_parallel``
    is the loop for those)."""
    log_interval, log_keys = _log_arguments('fit', log_interval, log_keys)
    if getattr(ts, 'world', 1) > 1:
        raise NotImplementedError(f'fit: a DataParallelTrainStep of world {ts.world} is not implemented: checkpoints and the evaluation '
                                  f'belong to rank 0 and need a barrier (train.fit_parallel is the loop for a process group)')
    eval_run = _fit_arguments('fit', eval_by, eval_run, eval_data)
    if _resume(ts, root, resume) and data_state:
        _resume_data(loader, root)
    log = _make_log(ts, loader, root, num_epochs, log_interval, log_keys, on_line)
    results = []

    def evaluate_at(ct):
        if log is not None:
            log.drain()
        checkpoint(ts, root)
        if data_state:
            _checkpoint_data(root, [loader.state()])
        if eval_run > 0 and ct % eval_run == 0:
            counter = evaluate(ts, evaluator, eval_data)
            with open(os.path.join(root, f'eval_{ts.epoch}_{ts.itr}.txt'), 'w') as fh:
                fh.write(counter.report())
            results.append((ts.epoch, ts.itr, counter.metrics()))

    _fit_loop(ts, loader, num_epochs, eval_by, eval_run, evaluate_at, log)
    return results


DATA_STATE = os.path.join('states', 'data_last.pth')


def _make_log(ts, loader, root, num_epochs, log_interval, log_keys, on_line):
    """the ``StepLog`` of a fit, or None with ``log_interval == 0``"""
    if log_interval == 0:
        return None
    num_epochs = int(ts.opt['train']['epochs'] if num_epochs is None else num_epochs)
    os.makedirs(root, exist_ok=True)
    return StepLog(ts, num_epochs * len(loader), os.path.join(root, 'log.txt'), log_interval, log_keys, on_line=on_line)


def _checkpoint_data(root, states):
    """``<root>/states/data_last.pth``: the ``TrainLoader.state()`` of every rank, in rank order"""
    os.makedirs(os.path.join(root, 'states'), exist_ok=True)
    torch.save({'world_size': len(states), 'ranks': list(states)}, os.path.join(root, DATA_STATE))


def _gather_data_states(loader, rank, world, group):
    """``loader.state()`` of every rank, in rank order, on rank 0 and None on the others: one ``gather_object`` where the group has
    several ranks (every rank calls this), nothing collective on one"""
    if world == 1:
        return [loader.state()]
    import torch.distributed as dist
    states = [None] * world if rank == 0 else None
    dist.gather_object(loader.state(), states, dst=0 if group is None else dist.get_global_rank(group, 0), group=group)
    return states


def _resume_data(loader, root, rank=0, world=1):
    """this rank's entry of ``states/data_last.pth`` into ``loader``, where the file exists (a run resumed from checkpoints that were
    written without ``data_state`` starts its streams over, as before)"""
    path = os.path.join(root, DATA_STATE)
    if not os.path.exists(path):
        return
    saved = torch.load(path, map_location='cpu', weights_only=False)
    if saved['world_size'] != world:
        raise ValueError(f'{path} holds the data streams of {saved["world_size"]} ranks, this run has {world}')
    loader.load_state(saved['ranks'][rank])


def _fit_arguments(who, eval_by, eval_run, eval_data):
    """the argument checks ``fit`` and ``fit_parallel`` share -> eval_run as an int"""
    if eval_by not in EVAL_BY:
        raise ValueError(f'{who}: eval_by = {eval_by!r} (one of {EVAL_BY})')
    eval_run = int(eval_run)
    if eval_run < 0 or (eval_run > 0 and eval_data is None):
        raise ValueError(f'{who}: eval_run = {eval_run} needs eval_run >= 0 and, to evaluate, eval_data')
    return eval_run


def _resume(ts, root, resume):
    """train.py:66-69: both ``last.pth`` files into ``ts`` where both exist and ``resume`` says so -> whether they were loaded"""
    last = os.path.join(root, 'models', 'last.pth'), os.path.join(root, 'states', 'last.pth')
    if resume and all(os.path.exists(p) for p in last):
        ts.load_state(*(torch.load(p, map_location='cpu', weights_only=False) for p in last))
        return True
    return False


def _fit_loop(ts, loader, num_epochs, eval_by, eval_run, evaluate_at, log=None):
    """the loop of ``Trainer.run`` (worker_v2.py:307-347): ``evaluate_at(ct)`` where the reference calls ``evaluate(ct)``, ``log``
    (a ``StepLog`` or None) updated after every step and closed at the end"""
    num_epochs = int(ts.opt['train']['epochs'] if num_epochs is None else num_epochs)
    while ts.epoch < num_epochs:
        if eval_by == 'itr':
            for batch, targets in loader.epoch(ts.epoch):
                out = ts.step(batch, targets)
                if log is not None:
                    log.update(out)
                if eval_run > 0 and ts.itr % eval_run == 0:          # worker_v2.py:340
                    evaluate_at(ts.itr)
            ts.epoch += 1
        else:
            run_epoch(ts, loader, log=log)
            evaluate_at(ts.epoch)                                    # worker_v2.py:345-347
    if log is not None:
        log.close()


EvalResult = namedtuple('EvalResult', 'epoch itr metrics loss')


def fit_parallel(ts, loader, root, num_epochs=None, evaluator=None, eval_data=None, eval_by='epoch', eval_run=0, resume=True,
                 val_loss=False, eval_shard=True, log_interval=0, log_keys=('cls', 'reg', 'total'), on_line=None, data_state=False):
    """``fit`` on a ``TrainStep`` or a ``DataParallelTrainStep`` of any world: ``Trainer.run`` under DistributedDataParallel.  The
    arguments of ``fit`` and two more.  ``val_loss=True``: every evaluation also computes the validation loss ``Evaluator.run`` logs, on
    the device (``evaluator.DeviceLossMeter``; ``eval_data`` is then a ``data.EvalBank``).  ``eval_shard``: below.
    -> [EvalResult(epoch, itr, metrics, loss)], ``loss`` None or {'cls_loss', 'reg_loss'} as Python floats.  The report file is
    ``counter.report()``, followed with ``val_loss=True`` by the loss line as the reference forms it (worker_v2.py:903-906).
    With a world-1 step and ``val_loss=False`` the loop launches and writes exactly what ``fit`` does, with the log and the data
    state on in both as well.
    ``log_interval`` / ``log_keys`` / ``on_line`` / ``data_state``: as in ``fit``.

    With a world above 1 (``ts.group`` is the process group; every rank calls this with the same arguments):
      * Refused with ValueError before anything is launched: a ``loader`` whose ``rank`` / ``world_size`` are not those of the group;
        ``skip_nonfinite=True`` without ``agree_skips=True`` (over many epochs a rank that skips alone parts from the others);
        ``eval_run > 0`` without ``eval_data``.
      * Resume: every rank loads both ``last.pth`` files, then a barrier (worker_v2.py:273-275).
      * Checkpoint: rank 0 alone calls ``ts.state()`` and writes the three files; the other ranks write nothing and read nothing back.
        Then a barrier, as in ``Trainer.evaluate`` (worker_v2.py:359-364).
      * ``eval_shard=True``: rank r evaluates the videos ``dist.assign_units(clips per video, world)[r]`` of the ``EvalBank``
        (``EvalBank.subset``) into its own ``DeviceRecallCounter`` and, with ``val_loss``, its own ``DeviceLossMeter``; the counter's
        int64 table and the meter's fp32 row table are then each summed over the ranks with ONE all-reduce (``dist._all_reduce_sum``:
        nccl on the device, gloo staged through the host).  Integer sums are exact and every row of the loss table is non-zero on one
        rank at most, so every rank holds the tables of one pass over the whole set and returns the same results; rank 0 writes
        ``eval_{epoch}_{itr}.txt``.  The EMA copies are bit-equal over the ranks, so this is the evaluation of one model.
      * ``eval_shard=False``: rank 0 evaluates alone and the others wait at the barrier, as the reference does; they return no
        results.
      * Every rank issues the same collectives in the same order: the step's own, then a barrier per checkpoint, then at most two
        all-reduces per evaluation.
      * The log: rank 0 alone owns a ``StepLog``, and it logs its own losses, as the reference does ("only track loss from rank 0 to
        avoid sync overhead"): no collective is added, and the other ranks construct and launch nothing.
      * ``data_state=True``: at every checkpoint ``loader.state()`` of every rank is gathered to rank 0 (one ``gather_object``, issued
        by every rank before the checkpoint's barrier) and written as one entry per rank; on resume every rank reads its own entry.
      * The one-pass LayerNorm guard (``GroundingEvaluator._run_on_device``): a rank whose guard trips resets its own counter and meter
        and repeats its own share before the reduce.  The two-pass repeat therefore covers a share, not the whole set: after a trip
        the videos of the other shares were evaluated with one-pass launches, and results may differ in the last bits between world
        sizes.

    Not here: W&B itself, losses reduced over the ranks, AMP."""
    from . import data as _data, evaluator as E
    world = getattr(ts, 'world', 1)
    group = getattr(ts, 'group', None)
    log_interval, log_keys = _log_arguments('fit_parallel', log_interval, log_keys)
    eval_run = _fit_arguments('fit_parallel', eval_by, eval_run, eval_data)
    rank = 0
    if world > 1:
        import torch.distributed as dist
        rank = dist.get_rank(group)
        if (getattr(loader, 'rank', None), getattr(loader, 'world_size', None)) != (rank, world):
            raise ValueError(f'fit_parallel: the loader is rank {getattr(loader, "rank", None)} of {getattr(loader, "world_size", None)}, the '
                             f'step\'s group makes this rank {rank} of {world}: TrainLoader(rank=, world_size=) shards the training data')
        if ts.skip_nonfinite and not getattr(ts, 'agree_skips', False):
            raise ValueError('fit_parallel: skip_nonfinite=True on several ranks needs agree_skips=True: the conv-gradient word is '
                             'rank-local, and a rank that skips alone parts from the others for the rest of the run')
    sharded = world > 1 and bool(eval_shard)
    if eval_run > 0 and (val_loss or sharded) and not isinstance(eval_data, _data.EvalBank):
        raise ValueError(f'fit_parallel: {"val_loss=True" if val_loss else "eval_shard=True"} evaluates a data.EvalBank on the device, '
                         f'eval_data is {type(eval_data).__name__}')
    barrier = (lambda: dist.barrier(group)) if world > 1 else (lambda: None)
    if _resume(ts, root, resume) and data_state:
        _resume_data(loader, root, rank, world)
    if resume:
        barrier()                                                    # worker_v2.py:273-275
    log = _make_log(ts, loader, root, num_epochs, log_interval, log_keys, on_line) if rank == 0 else None
    share = eval_data
    if sharded and eval_run > 0:
        clips = [eval_data.rows['vid'][k][1] for k in eval_data.index]
        share = eval_data.subset(D.assign_units(clips, world)[rank])
    meter = E.DeviceLossMeter(eval_data, ts.opt) if val_loss and eval_run > 0 else None
    results = []

    def evaluate_at(ct):
        if log is not None:
            log.drain()
        if rank == 0:
            checkpoint(ts, root)
        if data_state:
            states = _gather_data_states(loader, rank, world, group)
            if rank == 0:
                _checkpoint_data(root, states)
        due = eval_run > 0 and ct % eval_run == 0
        if due and sharded:                                          # every rank its share, after the checkpoint's barrier
            barrier()
            counter = evaluate(ts, evaluator, share, meter=None if meter is None else meter.reset())
            D._all_reduce_sum(counter._table, group, ts._backend)
            if meter is not None:
                D._all_reduce_sum(meter.rows, group, ts._backend)
            report(counter)
            return
        if due and rank == 0:                                        # worker_v2.py:359-364: rank 0 alone, the others wait
            report(evaluate(ts, evaluator, eval_data, meter=None if meter is None else meter.reset()))
        barrier()

    def report(counter):
        loss = None if meter is None else meter.losses()
        if rank == 0:
            with open(os.path.join(root, f'eval_{ts.epoch}_{ts.itr}.txt'), 'w') as fh:
                fh.write(counter.report() + ('' if loss is None else E.DeviceLossMeter.line(loss)))
        results.append(EvalResult(ts.epoch, ts.itr, counter.metrics(), loss))

    _fit_loop(ts, loader, num_epochs, eval_by, eval_run, evaluate_at, log)
    return results


class DataParallelTrainStep(TrainStep):
    """``TrainStep`` on every rank of ``process_group`` (None: one rank), each rank on its own share of the batch: the reference's
    Trainer with its model in DistributedDataParallel.  The world size comes from the group and reaches the objective as before.

    Construction broadcasts the parameters and buffers of the model and of the EMA copy from rank 0.  ``step`` differs from
    ``TrainStep.step`` in three places.  The earlier micro-batches accumulate locally (the reference's ``no_sync()``); only the LAST
    backward runs with the reducer armed: bucket by bucket the accumulated gradients are packed times 1 / world into one flat arena
    (dcf_dist_pack_grads) and all-reduced while the backward goes on, and afterwards every ``p.grad`` is its slice of the arena, the
    gradient averaged over the ranks.  The step's norm is summed over the ranks with one all-reduce of the device scalar before the
    loss-norm update.  The returned cls / reg / total stay rank-local (the reference logs rank 0 alone); grad_norm is the norm of the
    averaged gradient, equal on all ranks.

    A departure from the single-rank step: every parameter has a gradient after the reduce, zero if nothing reached it on any rank,
    so it takes weight decay and its Adam step count advances (``dist.GradReducer``).

    Dropout: the step does not touch the keys.  Ranks that should drop different elements pass different seeds, for example
    ``model.enable_dropout(seed=seed + rank)``.

    ``skip_nonfinite=True``: every rank owns a guard and decides for itself, with no further collective.  The verdict is taken from
    the norm of the AVERAGED gradient, which has the same bits on every rank, and a NaN or inf in one rank's share is one in the sum:
    all ranks skip the same steps and their parameters stay equal.  The conv-gradient word is rank-local; a non-finite sum it reports
    sits in a gradient of that rank and so in the average, except where a later mask multiplies it away -- then that rank alone would
    skip and the ranks would part.  Equal ``skipped`` counts in ``guard.report()`` of all ranks show that it has not happened.

    ``agree_skips=True`` closes that hole (with ``skip_nonfinite=True`` and a world above 1; otherwise it launches nothing): the
    loss-norm all-reduce carries two floats instead of one, [norm, flag].  Before it dcf_guard_word_publish writes 1.0 into the flag
    where this rank's conv-gradient word is set, after it dcf_guard_word_merge ORs ``DCF_GUARD_REMOTE`` into the word where the summed
    flag is not zero (include/decafnet_hip_fit.h).  The guarded norm that follows then skips on every rank and records the bit in
    ``conv_flag``.  The number of collectives is unchanged, and so is the norm: a count of positive points, summed as fp32, which is exact
    below 2^24 points per step over all ranks.  ``False`` -- the default -- launches exactly what
    was launched before the option existed.

    ``device_count=True``: as in ``TrainStep``; every rank keeps its own counts, which agree as long as the verdicts do.
    ``expert`` / ``expert_fn``: as in ``TrainStep``; every rank selects the clips of its own micro-batches.

    Backends: nccl (RCCL), one GPU per rank; gloo stages every bucket through the host and is a flow check for a one-GPU box."""

    def __init__(self, model, opt, itrs_per_epoch=1, process_group=None, bucket_bytes=D.DEFAULT_BUCKET_BYTES, front_end='dense',
                 skip_nonfinite=False, device_count=False, agree_skips=False, expert='dense', expert_fn=None):
        if not isinstance(agree_skips, bool):
            raise ValueError(f'DataParallelTrainStep: agree_skips = {agree_skips!r} (True or False)')
        self.agree_skips = agree_skips
        self.group = process_group
        self.world, self._backend = D._group_info(process_group)
        super().__init__(model, opt, world_size=self.world, itrs_per_epoch=itrs_per_epoch, front_end=front_end,
                         skip_nonfinite=skip_nonfinite, device_count=device_count, expert=expert, expert_fn=expert_fn)
        D.broadcast_module(model, 0, process_group)
        D.broadcast_module(self.ema.module, 0, process_group)
        self.reducer = D.GradReducer(self._params, process_group, bucket_bytes)

    def _backward(self, total, last):
        if not last:
            return total.backward()
        self.reducer.arm()
        try:
            total.backward()
        finally:
            self.reducer.disarm()
        self.reducer.finalize()

    def _norm_over_ranks(self, norm):
        if self.world > 1 and self.agree_skips and self.guard is not None:
            # [norm, flag]: the same collective, one float more.  The norm is a count of positive points that the objective formed in
            # fp32; fp32 adds integers exactly below 2^24, so the sum is the integer sum it was
            lib, st, state = _lib.lib(), _lib.current_stream(), self.guard._on(norm.device)
            pair = torch.empty(2, dtype=torch.float32, device=norm.device)
            pair[0].copy_(norm.reshape(()))
            _lib.check(lib.dcf_guard_word_publish(state, _lib.ptr(pair[1:]), st), 'dcf_guard_word_publish')
            D._all_reduce_sum(pair, self.group, self._backend)
            _lib.check(lib.dcf_guard_word_merge(state, _lib.ptr(pair[1:]), st), 'dcf_guard_word_merge')
            return pair[0].to(norm.dtype).reshape(norm.shape)
        if self.world > 1:
            norm = norm.clone()
            D._all_reduce_sum(norm, self.group, self._backend)
        return norm
