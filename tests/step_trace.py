"""What a fused training step ISSUES, in order: a recorder and the cases of tests/test_gpu_step_trace.py.

`with StepTrace() as t:` records, in the order they happen,
  ["call", entry point, [arguments]]   every C ABI call through the loaded library: ints and floats as passed, a pointer as
                                       "ptr" / "null", the stream argument (the last pointer of a launch) as "s<ordinal>";
                                       the two grouped weight-gradient launches also list their job tables' sizes
  ["wait_stream" | "wait_event" | "record", ...]   torch.cuda.Stream.wait_stream / wait_event and torch.cuda.Event.record
  ["alloc", function, shape, dtype, stream]        torch.empty / empty_like / zeros / ones / cat (stream: the current one)
  ["collective", name]                             torch.distributed collectives
  ["mark", label]                                  t.mark(label), the cases' own call boundaries
Streams and events are ordinals in order of first appearance, so two recordings of the same issue order are equal lists
whatever the addresses were.  A captured step replays without Python: equal recordings of its capture are the same graph.

The golden tests/golden/g28_fused_step_traces.json holds the recordings of CASES on the commit named inside it; nothing here
rewrites it (python tests/step_trace.py OUT.json COMMIT is how it was made there); tests/golden/g29_modular_step_traces.json holds
those of MODULAR_CASES, what the autograd Functions of evae/ops.py issue (... OUT.json COMMIT modular).  Every case is recorded on its second run behind a
fresh set of named workspaces (record() below): the first run leaves the workspaces, the one-element constants and the
zero-filled image buffers as an earlier step of the same shape leaves them, so a recording does not depend on what ran before."""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

# entry points whose last pointer is not a stream
NO_STREAM = {"evae_host_dedup", "evae_ctl_upload", "evae_cw_res_supported", "evae_conv2d_cl_res_supported"}
COLLECTIVES = ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "reduce", "reduce_scatter", "reduce_scatter_tensor",
               "all_to_all", "all_to_all_single", "barrier")
ALLOCS = ("empty", "empty_like", "zeros", "ones", "cat")
D, H, Z, B, N = 784, 300, 40, 16, 1000


class StepTrace:
    def __init__(self):
        self.records = []
        self._streams = {}       # raw handle -> ordinal
        self._events = []        # the event objects themselves (kept: an id must not be handed out twice)
        self._saved = []

    # ---- ordinals
    def _s(self, handle):
        return self._streams.setdefault(int(handle or 0), len(self._streams))

    def _cur(self):
        return self._s(torch.cuda.current_stream().cuda_stream)

    def _e(self, ev):
        for i, e in enumerate(self._events):
            if e is ev:
                return i
        self._events.append(ev)
        return len(self._events) - 1

    def mark(self, label):
        self.records.append(["mark", label])

    # ---- the C ABI
    def _call(self, name, argtypes, a):
        from evae import _lib
        out = []
        for i, (t, v) in enumerate(zip(argtypes, a)):
            if t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer)):
                raw = v.value if isinstance(v, C.c_void_p) else v
                if t is C.c_void_p and i == len(argtypes) - 1 and name not in NO_STREAM:
                    out.append("s%d" % self._s(raw))
                else:
                    out.append("ptr" if raw else "null")
            else:
                v = getattr(v, "value", v)
                out.append(int(v) if isinstance(v, (bool, int, np.integer)) else float(v))
        rec = ["call", name, out]
        table = {"evae_dense_bwd_weight_group": (_lib.WgradJob, ("M", "N", "K", "ldy", "ldx", "accumulate")),
                 "evae_dense_bwd_weight_finish_group": (_lib.WgradFinishJob, ("byte_rows", "M", "N", "K", "ldy", "ldx", "x_scale"))}.get(name)
        if table is not None:
            arr = C.cast(a[0], C.POINTER(table[0]))
            rec.append([[getattr(arr[j], f) for f in table[1]] for j in range(int(a[1]))])
        self.records.append(rec)

    def _patch(self, obj, name, new):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)

    def __enter__(self):
        from evae import _lib
        lib = _lib.load()
        for name, (_, argtypes) in _lib.SIGNATURES.items():
            fn = getattr(lib, name)

            def proxy(*a, _fn=fn, _name=name, _types=argtypes):
                self._call(_name, _types, a)
                return _fn(*a)
            self._patch(lib, name, proxy)

        Stream, Event = torch.cuda.streams.Stream, torch.cuda.streams.Event      # (the classes themselves: _distinct_streams)
        wait_stream, wait_event, record = Stream.wait_stream, Stream.wait_event, Event.record

        def p_wait_stream(st, other):
            self.records.append(["wait_stream", self._s(st.cuda_stream), self._s(other.cuda_stream)])
            return wait_stream(st, other)

        def p_wait_event(st, ev):
            self.records.append(["wait_event", self._s(st.cuda_stream), self._e(ev)])
            return wait_event(st, ev)

        def p_record(ev, stream=None):
            self.records.append(["record", self._e(ev), self._cur() if stream is None else self._s(stream.cuda_stream)])
            return record(ev) if stream is None else record(ev, stream)
        self._patch(Stream, "wait_stream", p_wait_stream)
        self._patch(Stream, "wait_event", p_wait_event)
        self._patch(Event, "record", p_record)
        for name in ALLOCS:
            def p_alloc(*a, _fn=getattr(torch, name), _name=name, **kw):
                t = _fn(*a, **kw)
                self.records.append(["alloc", _name, list(t.shape), str(t.dtype), self._cur() if t.is_cuda else "cpu"])
                return t
            self._patch(torch, name, p_alloc)
        import torch.distributed as dist
        for name in COLLECTIVES:
            if hasattr(dist, name):
                def p_coll(*a, _fn=getattr(dist, name), _name=name, **kw):
                    self.records.append(["collective", _name])
                    return _fn(*a, **kw)
                self._patch(dist, name, p_coll)
        return self

    def __exit__(self, *exc):
        for obj, name, old in reversed(self._saved):
            setattr(obj, name, old)
        self._saved = []
        return False


def calls(records, name):
    return [r for r in records if r[0] == "call" and r[1] == name]


# ------------------------------------------------------------------------------------------------ the cases
@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _exemplar_model(C_, seed, batch=B, **kw):
    import evae_oracle as orc
    import golden_inputs as gi
    import smoke_case
    args = smoke_case.vae_args(number_components=C_, training_set_size=N, batch_size=batch, **kw)
    if args.prior == "exemplar_prior" and args.model_name == "vae":
        model, _ = smoke_case.build_model(torch, np, orc, args)
    else:
        from utils.utils import importing_model
        torch.manual_seed(seed)
        model = importing_model(args)(args).cuda()
    model.train()
    data = gi.binary_images(seed, N)
    dataset = torch.utils.data.TensorDataset(torch.from_numpy(data), torch.arange(N).reshape(-1, 1), torch.zeros(N))
    return args, model, data, dataset


def _eager(t, C_=200, average=False, approx_k=None):
    kw = dict(approximate_prior=True, approximate_k=approx_k) if approx_k else {}
    args, model, data, dataset = _exemplar_model(C_, 28, **kw)
    eps = torch.from_numpy(np.random.RandomState(29).standard_normal((B, Z)).astype(np.float32)).cuda()
    model._draw_eps = lambda like: eps
    cache = None
    if approx_k:
        with torch.no_grad():
            cache = tuple(model.cache_z(dataset))
    xb = torch.from_numpy(data[:B]).cuda()
    ib = torch.arange(B).reshape(-1, 1).cuda()
    torch.manual_seed(30)
    torch.cuda.synchronize()
    with t:
        t.mark("forward")
        loss, RE, KL = model.calculate_loss((xb, ib), 0.5, average=average, dataset=dataset, cache=cache)
        assert "VaeExactLoss" in type(loss.grad_fn).__name__
        t.mark("backward")
        (loss if average else loss.sum()).backward()
    torch.cuda.synchronize()


def _graphed(t, C_=200, prior="exemplar_prior"):
    """five calls of a captured-step runner: the reference-form eager step, the captured form issued eagerly, the capture (+ its
    first replay), two more replays"""
    from evae.graph import GraphedTrainStep
    from utils.optimizer import AdamNormGrad
    args, model, data, dataset = _exemplar_model(C_, 31, prior=prior)
    opt = AdamNormGrad(model.parameters(), lr=5e-4)
    torch.manual_seed(32); torch.cuda.manual_seed(32)
    runner = GraphedTrainStep(model, opt, dataset, B, False, warmup_steps=2)
    torch.cuda.synchronize()
    with t:
        for it in range(5):
            t.mark("call %d" % it)
            runner(torch.from_numpy(data[it * B:(it + 1) * B]), torch.arange(it * B, (it + 1) * B).reshape(-1, 1), 0.5)
            if it == 1:
                assert runner.graph is None
    torch.cuda.synchronize()
    assert runner.graph is not None and not runner.failed and runner.replays == 3


def _graphed_p6(t):
    from evae import ops
    ops.gemm_x6_configure(1, 0)
    try:
        _graphed(t, C_=256)
    finally:
        ops.gemm_x6_configure(1, 2048)      # (the default policy, as tests/conftest.py restores it; -1 would leave it as set)


def std_refused_rows():
    """the smallest power-of-two batch the one-launch latent kernels of the standard-prior step refuse at the model's widths"""
    from evae import _lib
    lib = _lib.load()
    rows = B
    while lib.evae_heads_std_applies(rows, H, Z, H):
        rows *= 2
        assert rows <= 1 << 16
    return rows


def _std_eager(t, rows=B):
    import golden_inputs as gi
    args, model, data, dataset = _exemplar_model(1, 33, batch=rows, prior="standard")
    eps = torch.from_numpy(np.random.RandomState(34).standard_normal((rows, Z)).astype(np.float32)).cuda()
    model._draw_eps = lambda like: eps
    xb = torch.from_numpy(gi.binary_images(35, rows)).cuda()
    ib = torch.arange(rows).reshape(-1, 1).cuda()
    torch.cuda.synchronize()
    with t:
        t.mark("forward")
        loss, RE, KL = model.calculate_loss((xb, ib), 0.5, average=False)
        assert "VaeStandardLoss" in type(loss.grad_fn).__name__
        t.mark("backward")
        loss.sum().backward()
    torch.cuda.synchronize()


def _with_env(fn, **env):
    def run(t):
        with _env(**env):
            fn(t)
    return run


# name -> (run(trace), standard-prior step?)
CASES = {
    "eager_u8": (_eager, False),
    "eager_fp32": (_with_env(_eager, EVAE_U8_STORE="0"), False),
    # (C = 200 draws from 1000 rows are not worth distinct-row tables and a step that thin uploads its control block directly:
    #  the distinct-rows prior launch and the handing-over prologue need more draws and the staged upload)
    "graphed_rows_c1000": (_with_env(lambda t: _graphed(t, C_=1000), EVAE_CTL_DIRECT="0"), False),
    "graphed_every_draw": (_with_env(_graphed, EVAE_DEDUP="0"), False),
    "graphed_p6": (_graphed_p6, False),
    "graphed_merge_0": (_with_env(_graphed, EVAE_NODE_MERGE="0"), False),
    "graphed_merge_15": (_with_env(_graphed, EVAE_NODE_MERGE="15"), False),
    "eager_approx_k10": (lambda t: _eager(t, average=True, approx_k=10), False),
    "std_graphed": (lambda t: _graphed(t, C_=1, prior="standard"), True),
    "std_eager": (_std_eager, True),
    "std_eager_refused": (lambda t: _std_eager(t, std_refused_rows()), True),
}


# ------------------------------------------------------------------------------------------------ the modular operators' cases
def _hvae2(t):
    """one eager training step of hvae_2level on evae.ops' autograd Functions, as utils/training.py issues it"""
    from evae import ops
    args, model, data, dataset = _exemplar_model(200, 36, model_name="hvae_2level")
    xb = torch.from_numpy(data[:B]).cuda()
    ib = torch.arange(B).reshape(-1, 1).cuda()
    torch.manual_seed(37); torch.cuda.manual_seed(37)       # (the exemplar draws decide how many distinct rows are encoded)
    torch.cuda.synchronize()
    with t:
        t.mark("forward")
        loss, RE, KL = model.calculate_loss((xb, ib), 0.5, average=False, dataset=dataset)
        t.mark("backward")
        with ops.deferred_wgrads(loss):
            loss.sum().backward()
            t.mark("deferred")
    torch.cuda.synchronize()


def _hvae2_leaf(t):
    """(models/AbsHModel.py reads EVAE_HVAE_LEAF_STREAM once, at import: the case sets what that read leaves behind as well)"""
    import models.AbsHModel as hm
    old, hm._LEAF_STREAM = hm._LEAF_STREAM, True
    try:
        with _env(EVAE_HVAE_LEAF_STREAM="1"):
            _hvae2(t)
    finally:
        hm._LEAF_STREAM = old


# (N, C, H, W, Co, k, stride, pad), gated?, Hardtanh on the plain layer?, x.requires_grad?  Which family a geometry runs on is the
# library's answer (evae_conv2d_cl_supported): the first four rows -- rows of tests/test_gpu_conv.py's tables -- all run on the
# channels-last kernels, weight AND data gradient; the rows behind them take the other branches of Conv2dFn.backward
CONV_LAYERS = (((5, 1, 28, 28, 32, 3, 1, 1), True, False, False),           # a thin first layer: patch matrix + dense GEMM
               ((5, 32, 28, 28, 32, 3, 2, 1), True, False, False),
               ((5, 32, 28, 28, 32, 3, 2, 1), False, True, False),          # the activation's derivative written into dy
               ((7, 64, 7, 7, 6, 3, 1, 1), True, False, True),              # with the data gradient
               ((5, 32, 28, 28, 32, 3, 2, 1), False, False, False),         # plain, no activation: dy is the upstream gradient itself
               # 8 channels and 72 taps: neither a patch matrix nor the channels-last GEMM -- the NCHW family (the layers of
               # test_conv2d_activations_and_modules)
               ((4, 8, 10, 10, 6, 3, 2, 1), True, False, False),
               ((4, 8, 10, 10, 5, 3, 1, 1), False, True, False),
               # channels-last forward, 10 / 5 gradient channels per pixel (zero-padded to 32 in dy): both gradients on the NCHW kernels
               ((2, 1, 9, 11, 5, 3, 2, 1), True, False, True),
               ((2, 1, 9, 11, 5, 3, 2, 1), False, True, False))


def _conv_layers(t):
    from evae import ops
    rs = np.random.RandomState(38)
    jobs = []
    for (n, c, h, w, co, k, s, p), gated, clamp, x_grad in CONV_LAYERS:
        x = torch.from_numpy(rs.standard_normal((n, c, h, w)).astype(np.float32)).cuda().requires_grad_(x_grad)
        prm = [torch.from_numpy((rs.standard_normal(shape) * 0.1).astype(np.float32)).cuda().requires_grad_(True)
               for shape in ((co, c, k, k), (co,), (co, c, k, k), (co,))]
        gout = torch.from_numpy(rs.standard_normal((n, co, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1)).astype(np.float32)).cuda()
        jobs.append((x, prm, gout, s, p, gated, clamp))
    torch.cuda.synchronize()
    with t:
        for i, (x, (wh, bh, wg, bg), gout, s, p, gated, clamp) in enumerate(jobs):
            t.mark("layer %d forward" % i)
            if gated:
                y = ops.gated_conv2d(x, wh, bh, wg, bg, s, p)
            else:
                y = ops.conv2d(x, wh, bh, s, p, *((ops.ACT_HARDTANH, -4.5, 0.0) if clamp else ()))
            t.mark("layer %d backward" % i)
            y.backward(gout)
    torch.cuda.synchronize()


@contextlib.contextmanager
def _ops_attr(name, value):
    from evae import ops
    old = getattr(ops, name)
    setattr(ops, name, value)
    try:
        yield
    finally:
        setattr(ops, name, old)


def _conv_stack(t):
    import test_gpu_conv as tc
    n = 37
    net = tc._stack(tc._NARROW, 3).cuda()
    rs = np.random.RandomState(n)
    x = torch.from_numpy((rs.rand(n, 1, 28, 28) < 0.3).astype(np.float32)).cuda()
    gout = torch.from_numpy(rs.standard_normal((n, 6, 7, 7)).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    with _ops_attr("CONV_STACK_MIN_IMAGES", 1), t:
        t.mark("forward")
        y = net(x)
        t.mark("backward")
        y.backward(gout)
    torch.cuda.synchronize()


def _res_run(t):
    from evae import ops
    n, c, h, nblk = 9, 48, 14, 2
    rs = np.random.RandomState(n + c + h)
    x = torch.from_numpy((rs.standard_normal((n, c, h, h)) * 1.5).astype(np.float32)).cuda().requires_grad_(True)
    blocks = [(torch.from_numpy((rs.standard_normal((c, c, 3, 3)) / np.sqrt(c * 9)).astype(np.float32)).cuda().requires_grad_(True),
               torch.from_numpy((rs.standard_normal(c) * 0.1).astype(np.float32)).cuda().requires_grad_(True)) for _ in range(nblk)]
    gout = torch.from_numpy(rs.standard_normal((n, c, h, h)).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    with _ops_attr("RES_STACK_MIN_PIXELS", 1), t:
        t.mark("forward")
        y = ops.res_stack(x, blocks)
        t.mark("backward")
        y.backward(gout)
    torch.cuda.synchronize()


# name -> (run(trace),): what evae.ops' autograd Functions issue, recorded in tests/golden/g29_modular_step_traces.json
MODULAR_CASES = {
    "hvae2_u8": (_hvae2,),
    "hvae2_fp32": (_with_env(_hvae2, EVAE_U8_STORE="0"),),
    "hvae2_leaf": (_hvae2_leaf,),
    "conv_layers": (_conv_layers,),
    "conv_stack": (_conv_stack,),
    "res_run": (_res_run,),
}


class _Off:
    """the un-recorded first run of a case"""

    def mark(self, label):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@contextlib.contextmanager
def _distinct_streams():
    """torch hands its streams out of a pool of 32 per priority, round robin: the stream a runner makes for a warm-up call can BE
    the capture stream, or the model's side stream, depending on how many streams the process made before -- two roles on one
    ordinal in one recording and not in the next.  While a case runs, a new stream is drawn again until its handle is one no
    stream known so far has."""
    from evae import ops
    base = torch.cuda.streams.Stream
    known = list(ops._SIDE_STREAM_OBJS) + [getattr(torch.cuda.graph, "default_capture_stream", None)]
    taken = {0} | {int(s_.cuda_stream) for s_ in known if s_ is not None}

    class Distinct(base):
        def __new__(cls, *a, **kw):
            s_ = base.__new__(cls, *a, **kw)
            if "stream_id" not in kw and "stream_ptr" not in kw:
                for _ in range(64):
                    if int(s_.cuda_stream) not in taken:
                        break
                    s_ = base.__new__(cls, *a, **kw)
                taken.add(int(s_.cuda_stream))
            return s_
    torch.cuda.Stream = Distinct
    try:
        yield
    finally:
        torch.cuda.Stream = base


def record(name):
    """The case's recording, on its second run behind a fresh set of named workspaces: a launch is handed its workspace's whole
    size, and a workspace is as large as the largest request the process ever made under its name.  The buffers in use so far
    are retired (kept allocated: a captured graph of an earlier test may hold their addresses), not freed."""
    from evae import ops
    ops._ws_retired.extend(ops._ws.values())
    ops._ws.clear()
    run = (CASES.get(name) or MODULAR_CASES[name])[0]
    with _distinct_streams():
        run(_Off())
        t = StepTrace()
        run(t)
    return t.records


if __name__ == "__main__":
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (os.path.join(root, "exemplar-vae_amd"), os.path.join(root, "oracle"), here):
        sys.path.insert(0, p)
    out = {"commit": subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=root).decode().strip() if len(sys.argv) < 3 else sys.argv[2],
           "cases": {}}
    for name in (MODULAR_CASES if sys.argv[3:] == ["modular"] else CASES):       # OUT.json COMMIT modular: the g29 golden
        try:
            out["cases"][name] = record(name)
            print(name, len(out["cases"][name]), "records", flush=True)
        except Exception as e:      # a case that cannot be recorded on this commit is left out (and said so)
            print(name, "NOT RECORDED: %s: %s" % (type(e).__name__, e), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, separators=(",", ":"))
