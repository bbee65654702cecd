"""The launch plan of the model engines, recorded: which C entry points a train step calls, in which order, with which arguments.

The engines (mmif/engine.py, mmif/nest_engine.py) choose between kernel routes that are bit-identical by design, so no numeric test sees
WHICH route ran.  `record()` replaces every work-enqueuing attribute of mmif._lib.lib with a pass-through wrapper for the duration of a
case and notes each call: the function name, every scalar argument by value, every mmif_tensor (also those inside an MmifDenseChain) as
(dtype, n, h, w, halo, cb_total, cb_off, cb, flags), every other pointer as null / non-null.  Addresses are never recorded.  Host queries
(*_supported*, *_fits, *_workspace*, *_bytes*, mmif_get_*, ...) are not recorded: how often they are asked is not part of the plan.

CASES lists (id, model, call, dtype, impl, switch, steps); run_case() builds the model fresh, runs three steps
m(i1, i2).square().mean().backward() -- the first contains the operand packs, the second is the steady state, the third follows a
WEIGHTS_EPOCH bump (the re-pack route) -- and returns the records of the steps the case keeps.  Shared by
tests/golden/make_golden_launch_plans.py (writes the fixture) and tests/test_gpu_launch_plan.py (compares with it)."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import re

_QUERY = re.compile(r"_supported|_fits$|_workspace|_bytes|^mmif_get_|^mmif_last_error$|^mmif_version$")
_SCALARS = (C.c_int32, C.c_uint64, C.c_float, C.c_size_t, C.c_int64, C.c_double)

DENSE_SWITCHES = ["MMIF_ENC_STREAM", "MMIF_ENC_BWD_FUSED", "MMIF_ENC_CHAIN", "MMIF_ENC_CHAIN_STREAM", "MMIF_ENC_WGRAD", "MMIF_BWD_PAIR",
                  "MMIF_BWD_WIDE", "MMIF_IMAGE_BWD", "MMIF_DEFER_REDUCE", "MMIF_FUSE_SHARE", "MMIF_ENC_SUM", "MMIF_DGRAD_DUP", "MMIF_PAIR_BWD"]
NON_DEFAULT = {s: "0" for s in DENSE_SWITCHES}
NON_DEFAULT["MMIF_DEFER_REDUCE"] = "1"      # (the one switch that is off by default)
FP32_SWITCHES = ["MMIF_ENC_WGRAD", "MMIF_ENC_CHAIN", "MMIF_BWD_WIDE"]
# (label, model class, two images?)
DENSE_MODELS = [("PFNetv1", "PFNetv1", True), ("VIFNet", "VIFNet", True), ("DenseFuse", "DenseFuse", True), ("DenseFuse1", "DenseFuse", False),
                ("PFNetv2", "PFNetv2", True)]
NEST_MODELS = ["NestFuse", "RFNNest"]
DENSE_SHAPE, NEST_SHAPE = (1, 1, 37, 53), (1, 1, 32, 32)
# 37 x 53 is too small for the asynchronous dgrad kernel (it wants two tiles of 16 x 16 per compute unit), so DenseFuse's shared-gradient
# and dup routes ('sum' fusion: share_fused_grad, dup_ok) never run there: the two-image DenseFuse also at the shape at which
# tests/test_gpu_enc_wgrad.py runs its train step on those routes
SHARE_SHAPE = (8, 1, 128, 128)
SHARE_SWITCHES = ["MMIF_DGRAD_DUP", "MMIF_FUSE_SHARE", "MMIF_ENC_BWD_FUSED", "MMIF_ENC_CHAIN_STREAM", "MMIF_ENC_CHAIN", "MMIF_ENC_WGRAD"]
ALL_STEPS, STEADY = (0, 1, 2), (1,)


def _cases():
    out = []
    for label, cls, two in DENSE_MODELS:
        arms = [("bf16", "auto", None)] + [("bf16", "auto", s) for s in DENSE_SWITCHES] + [("bf16", "valu", None), ("fp32", "auto", None)]
        arms += [("fp32", "auto", s) for s in FP32_SWITCHES] + [("fp32", "valu", None)]
        for dtype, impl, sw in arms:
            cid = f"{label}-{dtype}-{impl}-" + (f"{sw}={NON_DEFAULT[sw]}" if sw else "default")
            out.append(dict(id=cid, model=cls, two=two, shape=DENSE_SHAPE, dtype=dtype, impl=impl, switch=sw, steps=STEADY if sw else ALL_STEPS))
    for sw in [None] + SHARE_SWITCHES:
        cid = "DenseFuse@8x128x128-bf16-auto-" + (f"{sw}={NON_DEFAULT[sw]}" if sw else "default")
        out.append(dict(id=cid, model="DenseFuse", two=True, shape=SHARE_SHAPE, dtype="bf16", impl="auto", switch=sw, steps=STEADY if sw else ALL_STEPS))
    for cls in NEST_MODELS:
        for dtype in ("bf16", "fp32"):
            out.append(dict(id=f"{cls}-{dtype}-auto-default", model=cls, two=True, shape=NEST_SHAPE, dtype=dtype, impl="auto", switch=None,
                            steps=ALL_STEPS))
    return out


CASES = _cases()


def enqueue_names():
    """every C entry point that enqueues work: status-returning, the stream as its last argument (+ mmif_reduce_defer_begin, which
    redirects the launches that follow); host queries left out"""
    from mmif import _lib
    names = [n for n, (res, args) in _lib.SIGNATURES.items()
             if res is C.c_int32 and args and args[-1] is C.c_void_p and not _QUERY.search(n)]
    return names + ["mmif_reduce_defer_begin"]


def _tensor(t):
    return [t.dtype, t.n, t.h, t.w, t.halo, t.cb_total, t.cb_off, t.cb, t.flags]


def _nonnull(a):
    if a is None:
        return 0
    if isinstance(a, int):
        return int(a != 0)
    if isinstance(a, C.c_void_p):
        return int(bool(a.value))
    if isinstance(a, C._Pointer):
        return int(bool(a))
    return 1            # byref(...) / an array: the address of a live object


def _arg(a, argtype):
    from mmif import _lib
    if argtype in _SCALARS:
        v = a.value if hasattr(a, "value") else a
        return float(v) if argtype in (C.c_float, C.c_double) else int(v)
    if argtype in (C.POINTER(_lib.MmifTensor), C.POINTER(_lib.MmifDenseChain)) and a is not None:
        obj = a._obj if hasattr(a, "_obj") else a.contents           # byref(struct) or pointer(struct)
        if isinstance(obj, _lib.MmifTensor):
            return _tensor(obj)
        return {"g3": _tensor(obj.g3.contents) if obj.g3 else None, "glow": _tensor(obj.glow.contents) if obj.glow else None,
                "x": _tensor(obj.x.contents) if obj.x else None, "out": _tensor(obj.out.contents) if obj.out else None,
                "packed": [int(bool(p)) for p in obj.packed]}
    return "ptr" if _nonnull(a) else None


@contextlib.contextmanager
def record(calls):
    """while active, every enqueuing entry point of mmif._lib.lib appends [name, arg, ...] to `calls` and passes the call through"""
    from mmif import _lib
    lib = _lib.lib
    saved = {}

    def wrap(name, fn, argtypes):
        def f(*args):
            calls.append([name] + [_arg(a, t) for a, t in zip(args, argtypes)])
            return fn(*args)
        return f
    try:
        for name in enqueue_names():
            fn = getattr(lib, name)
            saved[name] = fn
            setattr(lib, name, wrap(name, fn, _lib.SIGNATURES[name][1]))
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


@contextlib.contextmanager
def settings(dtype, impl, env):
    """storage dtype, kernel family and $MMIF_... switches for the duration of a case (os.environ + reload_switches(), restored)"""
    from mmif import engine as E
    env = dict(env, MMIF_CONV_IMPL=impl)
    prev_dtype = E.compute_dtype()
    prev = {k: os.environ.get(k) for k in env}
    try:
        E.set_compute_dtype(dtype)
        os.environ.update(env)
        E.reload_switches()
        yield
    finally:
        E.set_compute_dtype(prev_dtype)
        for k, v in prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        E.reload_switches()


def run_case(case):
    """-> {step index: [call record, ...]} for the steps the case keeps"""
    import torch
    import core.model as M
    from mmif import engine as E
    env = {case["switch"]: NON_DEFAULT[case["switch"]]} if case["switch"] else {}
    with settings(case["dtype"], case["impl"], env):
        torch.manual_seed(5)
        m = getattr(M, case["model"])().to("cuda:0")
        g = torch.Generator(device="cpu").manual_seed(5)
        imgs = [torch.rand(case["shape"], generator=g).to("cuda:0") for _ in range(2 if case["two"] else 1)]
        steps = {}
        for step in range(3):
            if step == 2:
                E.WEIGHTS_EPOCH[0] += 1
            with record([]) as calls:
                m(*imgs).square().mean().backward()
            if step in case["steps"]:
                steps[step] = calls
        torch.cuda.synchronize()
    return steps


def canonical(call):
    return json.dumps(call, sort_keys=True, separators=(",", ":"))


def summarise(calls):
    """what the fixture holds per step: the ordered function names, a SHA-256 over the canonical full record, and 6 hex digits per call
    (of that call's own SHA-256) so that a mismatch can be pinned to its call"""
    lines = [canonical(c) for c in calls]
    return {"names": [c[0][len("mmif_"):] for c in calls],       # (every entry point starts with mmif_: left out of the fixture)
            "digest": hashlib.sha256("\n".join(lines).encode()).hexdigest(),
            "calls": "".join(hashlib.sha256(l.encode()).hexdigest()[:6] for l in lines)}
