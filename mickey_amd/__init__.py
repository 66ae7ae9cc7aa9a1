"""mickey_amd: MI355X-native implementation of the MicKey inference hot path
(DINOv2 encoder + heads -> dual-softmax matcher -> probabilistic-Procrustes RANSAC)."""
__version__ = "0.1.0"


def use_hip_training(model, blocks=False, **kw):
    """Every use_hip_* swap of a reference training model in one call: the frozen encoder, the 3x3 convs, the linear attention, the
    EncoderLayers, the head tails and the matcher -- and, with blocks=True, the BatchNorm / ReLU / shortcut glue of the BasicBlocks
    (use_hip_blocks; off by default: measured, it loses to the torch glue, profiles/train_block_bench.txt).  Keyword arguments go to the swaps that take
    them (use_hip_encoder: dtype, ln_fold, features_lp; use_hip_matcher: split); an unknown one is a TypeError.  Returns {name of
    the swap: its count}."""
    import inspect

    from . import train_attention, train_encoder, train_heads, train_layer, train_matcher, train_tails
    calls = (train_encoder.use_hip_encoder, train_heads.use_hip_convs, train_layer.use_hip_encoder_layers,
             train_attention.use_hip_attention, train_tails.use_hip_tails, train_matcher.use_hip_matcher)
    takes = [set(inspect.signature(f).parameters) - {"model"} for f in calls]
    unknown = set(kw) - set().union(*takes)
    if unknown:
        raise TypeError("use_hip_training: unexpected keyword arguments %s" % sorted(unknown))
    counts = {f.__name__: f(model, **{k: v for k, v in kw.items() if k in t}) for f, t in zip(calls, takes)}
    if blocks:
        from . import train_block
        counts["use_hip_blocks"] = train_block.use_hip_blocks(model)
    return counts
