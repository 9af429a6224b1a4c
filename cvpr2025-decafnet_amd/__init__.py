"""MI355X-native implementation of the DeCafNet grounding hot path.

The directory name is not a valid Python identifier; import it with
``importlib.import_module('cvpr2025-decafnet_amd')``.

Sub-modules: ``modeling`` (libs/modeling drop-in), ``nms`` (libs/nms drop-in), ``evaluator``
(the Evaluator hot-path harness), ``config`` / ``synth`` (plain-dict opt tree, synthetic data),
``data`` (feature files, text-CLS table, annotation file -> per-video dicts), ``dropin`` (runs the reference's own
``eval.py`` / ``Evaluator`` on this package without editing it), ``loss`` (libs/modeling/loss.py forward values), ``autograd`` (differentiable MaskedConv1D / channel LayerNorm / window attention /
cross attention / AdaLN modulation / depthwise convolution / max pooling / GELU / LayerScale residual, and heads, whole TransformerEncoder blocks, whole
TransformerDecoder layers and the XAttNFusion stack composed of them: ``cross_attention``, ``adaln_modulate``, ``xattn_mha``, ``conv_xattn_layer``, ``transformer_decoder``, ``xattn_fusion``; the refinement stage ``refine_in``, ``tcn_layer``, ``tcn`` and ``fuse_and_predict``; the two backbones
``video_transformer`` (with the k = 5 / stride-2 ``strided_masked_conv1d``) and ``text_transformer``), ``dist`` (T-sharding over ranks; the bucketed gradient all-reduce of data-parallel training), ``build`` (hipcc driver),
``_lib`` (ctypes binding of the C ABI), ``optim`` (the Trainer's update: gradient clipping, Adam / AdamW and the EMA copy as multi-tensor kernels,
the reference's parameter groups and schedulers), ``train`` (the differentiable training forward and ``TrainStep``, one whole iteration; ``DataParallelTrainStep``, the same on every rank of a process group).
"""
from . import config, synth  # noqa: F401


def __getattr__(name):
    # heavy sub-modules are imported on first use so that `config`/`synth` work without the .so
    if name in ('modeling', 'nms', 'evaluator', 'build', '_lib', 'dist', 'data', 'dropin', 'loss', 'autograd', 'optim', 'train'):
        import importlib
        return importlib.import_module(f'{__name__}.{name}')
    raise AttributeError(name)
