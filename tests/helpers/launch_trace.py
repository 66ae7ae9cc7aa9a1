"""The launch sequence of pipeline.heads_forward at the level of the C ABI, recorded on the CPU: no GPU, no kernel runs.

ops.* stays real; what ops imported from _native is replaced: `call` records, `ptr` returns an identity instead of an address,
`stream` returns 0, `sat_word` passes the saturation word on as such an identity (the real one asserts is_cuda); `query` stays
real (the library loads without a device).  One record per configuration (CONFIGS):

  calls    every mk_* call in order, [name, arg, ...]: a pointer is [ordinal, byte offset] -- the underlying storages numbered
           by first appearance in the trace, the offset of the tensor inside its storage --, None stays null, integers stay,
           floats are written with float.hex
  allocs   every Workspace.get request, in first-request order: [name, shape, dtype, zero]
  profile  the same run seen by bench.StageProfiler (wrapped around ops.* as bench.py --full does, HIP events stubbed): per
           stage launches, work and bytes -- bench.py's accounting lambdas name the parameters of the ops.* wrappers

tests/golden/heads_launch_trace.json holds the records of the pipeline.py the refactor of heads_forward started from;
tests/test_heads_trace_cpu.py compares the current heads_forward with it, ==, no tolerance.  To regenerate it from any commit:

  git show <commit>:mickey_amd/pipeline.py > pipeline_then.py
  python -m tests.helpers.launch_trace --pipeline pipeline_then.py --out trace_then.json

(--pipeline: that file is loaded as a sibling module of the package, beside the current ops / weights; default: the package's own
pipeline.py.  --out: default the committed file.)"""
import argparse
import copy
import importlib.util
import json
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RECORD = os.path.join(ROOT, "tests", "golden", "heads_launch_trace.json")
NIMG, GH, GW = 2, 5, 7   # non-square: a swapped H / W or a row count taken from the wrong grid shows

# name -> (encoder dtype, heads dtype, heads_split, features_lp, LINATTN_FUSED, KP_HEADS.POS_ENCODING, DSC_HEAD.POS_ENCODING)
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32
CONFIGS = {
    "fp16-fused": (f16, f16, False, False, True, True, True),
    "bf16-fused": (bf16, bf16, False, False, True, True, True),
    "fp16-unfused": (f16, f16, False, False, False, True, True),
    "fp32": (f32, f32, False, False, True, True, True),
    "split": (f16, f32, True, False, True, True, True),
    "split-flp": (f16, f32, True, True, True, True, False),
    "fp16-pe-mixed": (f16, f16, False, False, True, False, True),
}
_CACHE = {}   # the synthetic checkpoint and the prepared weights, shared between configurations


class _Ptr:
    def __init__(self, t):
        self.t = t   # (held: a storage that lives cannot hand its address to another one)


def load_pipeline(path=None):
    """The package's pipeline module, or the pipeline.py at `path` loaded as mickey_amd._traced_pipeline (its `from . import
    ops` finds the package's modules)."""
    if path is None:
        from mickey_amd import pipeline
        return pipeline
    import mickey_amd  # noqa: F401
    spec = importlib.util.spec_from_file_location("mickey_amd._traced_pipeline", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _weights(cfg, enc, heads, split, flp):
    from mickey_amd import synthetic as syn, weights
    if "sd" not in _CACHE:
        _CACHE["sd"] = syn.mickey_state_dict(cfg, seed=0, arch="vit_tiny_test")
    key = (enc, heads, split, flp)
    if key not in _CACHE:
        _CACHE[key] = weights.prepare(_CACHE["sd"], cfg, torch.device("cpu"), enc, heads_dtype=heads, heads_split=split,
                                      features_lp=flp)
    return _CACHE[key]


def trace(name, pipeline=None):
    """The record {calls, allocs, profile} of configuration `name`; pipeline: the module whose heads_forward runs."""
    import bench
    from mickey_amd import ops
    from mickey_amd.config import default_cfg
    pipeline = load_pipeline() if pipeline is None else pipeline
    enc, heads, split, flp, fused, kp_pe, dsc_pe = CONFIGS[name]
    cfg = copy.deepcopy(default_cfg())
    cfg["MICKEY"]["DINOV2"]["CHANNEL_DIM"] = 128
    cfg["AMD"]["LINATTN_FUSED"] = fused
    cfg["MICKEY"]["KP_HEADS"]["POS_ENCODING"] = kp_pe
    cfg["MICKEY"]["DSC_HEAD"]["POS_ENCODING"] = dsc_pe
    W = _weights(cfg, enc, heads, split, flp)
    calls, allocs, ordinals = [], [], {}

    def arg(v):
        if isinstance(v, _Ptr):
            base = v.t.untyped_storage().data_ptr()
            return [ordinals.setdefault(base, len(ordinals)), v.t.data_ptr() - base]
        if isinstance(v, float):
            return v.hex()
        if v is None or isinstance(v, int):
            return v
        raise TypeError("launch trace: argument of type %s" % type(v).__name__)

    class Workspace(pipeline.Workspace):
        def get(self, name, shape, dtype, device, zero=False):
            ent = [name, list(shape), str(dtype).replace("torch.", ""), bool(zero)]
            if ent[:3] not in [a[:3] for a in allocs]:
                allocs.append(ent)
            return super().get(name, shape, dtype, device, zero=zero)

    ws = Workspace()
    R = ops.bordered_rows(NIMG, GH, GW)
    if split:
        ws.sat_flag = torch.zeros((1,), dtype=torch.int32)
        planes = torch.zeros((2, R, W.D), dtype=f16)
        feat = (planes[0], planes[1])
    else:
        feat = torch.zeros((R, W.D), dtype=heads)
    prof = bench.StageProfiler()
    event = type("Event", (), {"record": lambda self: None, "elapsed_time": lambda self, other: 1.0})
    saved, ev = dict(vars(ops)), torch.cuda.Event
    try:
        ops.call, ops.stream = lambda fn, *a: calls.append([fn] + [arg(v) for v in a]), lambda: 0
        ops.ptr = ops.sat_word = lambda t: None if t is None else _Ptr(t)
        torch.cuda.Event = lambda enable_timing=True: event()
        prof.wrap(ops)
        prof.on = True
        pipeline.heads_forward(W, ws, feat, NIMG, GH, GW, cfg)
    finally:
        torch.cuda.Event = ev
        for k, v in saved.items():   # (the stand-ins and the profiler's wrappers come off again)
            setattr(ops, k, v)
    profile = {stage: {k: d[k] for k in ("launches", "work", "bytes")} for stage, d in sorted(prof.summary(1)[1].items())}
    return {"calls": calls, "allocs": allocs, "profile": profile}


def dumps(records):
    """One call / request / stage per line: the file diffs line by line."""
    out = []
    for name, rec in records.items():
        parts = []
        for part in ("calls", "allocs"):
            parts.append('  "%s": [\n%s\n  ]' % (part, ",\n".join("   " + json.dumps(e, separators=(",", ":")) for e in rec[part])))
        parts.append('  "profile": {\n%s\n  }' % ",\n".join('   "%s": %s' % (s, json.dumps(d)) for s, d in rec["profile"].items()))
        out.append(' "%s": {\n%s\n }' % (name, ",\n".join(parts)))
    return "{\n%s\n}\n" % ",\n".join(out)


def first_difference(part, got, want):
    """Plain text for an assertion message: the first entry of `part` where the two records part ways."""
    if isinstance(got, dict):
        got, want = sorted(got.items()), sorted(want.items())
    for i in range(max(len(got), len(want))):
        g, w = (got[i] if i < len(got) else None), (want[i] if i < len(want) else None)
        if g != w:
            where = ""
            if isinstance(g, list) and isinstance(w, list) and len(g) == len(w):
                where = " (argument %s)" % ", ".join(str(j) for j in range(len(g)) if g[j] != w[j])
            return "%s[%d]%s differs\n  now:    %s\n  record: %s" % (part, i, where, json.dumps(g), json.dumps(w))
    return "%s: equal" % part


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pipeline", default=None, help="trace the heads_forward of this pipeline.py (default: the package's own)")
    ap.add_argument("--out", default=RECORD)
    a = ap.parse_args()
    mod = load_pipeline(a.pipeline)
    text = dumps({name: trace(name, mod) for name in CONFIGS})
    with open(a.out, "w") as f:
        f.write(text)
    print("%s: %d configurations, %d bytes" % (a.out, len(CONFIGS), len(text)))


if __name__ == "__main__":
    main()
