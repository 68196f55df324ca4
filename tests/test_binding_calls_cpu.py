"""Pins what every hip_binding wrapper passes to the C ABI (no GPU, no built library).

`hb._lib` is replaced by a stub whose `fhvae_*` attributes record (symbol, rendered arguments) and return 0 (or what the case
sets for a host-side query), `hb._need_gpu` by a no-op, `hb._stream` by `lambda: 0`, `hb._device_words` by a CPU tensor and
`hb.OP_TIMER` by a recorder of the timing labels.  The cases drive the wrappers through CPU tensors: the kernels never run,
the outputs are uninitialised memory, and only the order of the calls and their arguments is compared with
tests/golden/binding_calls.json.

Rendering (argument kinds from hb.SIGNATURES): scalars by value; a NULL pointer `null`; a pointer into a tensor the case
registered `in:<k>+<byte offset>` (`in:<k>` at its start); any other pointer `new:<j>`, numbered by first appearance within the case (no address
reaches the golden file; the case keeps every tensor it makes alive, so no address is used twice); byref structs and ctypes
arrays of structs field by field in the same way, compactly: the first struct of a type in a case lists its fields that are not
NULL / 0 (pointer arrays without their trailing NULLs), every later one of that type only the fields that differ from the one
before it.  The descriptors are passed to several queries and launches in a row, so most renderings are `{}`: nothing changed.
Timing labels: `["+"]` where the op timer starts, `["-", label]` where it stops.  Cases with identical traces share one entry.

The golden file is produced by running this file as a script (`python tests/test_binding_calls_cpu.py --write`) and is only
ever regenerated from a hip_binding.py whose calls are known good: a refactor of the binding must pass against the file its
parent commit wrote.
"""
import contextlib
import ctypes as C
import json
import os
import sys

import pytest
import torch
from torch.overrides import TorchFunctionMode

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, "pytorch-scalablefhvae_amd") not in sys.path:  # (run as a script: no conftest)
    sys.path.insert(0, os.path.join(_ROOT, "pytorch-scalablefhvae_amd"))

import hip_binding as hb  # noqa: E402

GOLDEN = os.path.join(_ROOT, "tests", "golden", "binding_calls.json")
_FLOATS = (C.c_float, C.c_double)


class _KeepAlive(TorchFunctionMode):
    """Holds every result of a torch call made while it is active, so that no address is freed and handed out again."""

    def __init__(self):
        super().__init__()
        self.kept = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.kept.append(out)
        return out


class Trace:
    def __init__(self, ret=None):
        self.calls, self.inputs, self.new, self.ret, self.last = [], [], {}, dict(ret or {}), {}

    def ins(self, *ts):
        """Register the tensors a case passes in (None is skipped); returns them."""
        self.inputs.extend(t for t in ts if t is not None)
        return ts[0] if len(ts) == 1 else ts

    def n_calls(self):
        return sum(1 for c in self.calls if c[0].startswith("fhvae_"))

    def ptr(self, v):
        if v is None or int(v) == 0:
            return "null"
        v = int(v)
        for k, t in enumerate(self.inputs):
            st = t.untyped_storage()
            if st.data_ptr() <= v < st.data_ptr() + st.nbytes():
                return "in:%d+%d" % (k, v - st.data_ptr()) if v != st.data_ptr() else "in:%d" % k
        return "new:%d" % self.new.setdefault(v, len(self.new))

    def field(self, ftype, v):
        if issubclass(ftype, C.Structure):
            full = {n: self.field(t, getattr(v, n)) for n, t in ftype._fields_}
            prev = self.last.get(ftype.__name__)
            self.last[ftype.__name__] = {n: x for n, x in full.items() if not issubclass(dict(ftype._fields_)[n], C.Structure)}
            if prev is None:
                return {n: x for n, x in full.items() if x not in ("null", 0, [])}
            return {n: x for n, x in full.items() if prev.get(n, x) != x}
        if issubclass(ftype, C.Array):
            out = [self.field(ftype._type_, x) for x in v]
            while out and out[-1] == "null":
                out.pop()
            return out
        if ftype is C.c_void_p:
            return self.ptr(v)
        return float(v) if ftype in _FLOATS else int(v)

    def arg(self, kind, v):
        if hasattr(v, "_obj"):  # C.byref(struct)
            return self.field(type(v._obj), v._obj)
        if isinstance(v, C.Array):
            et = v._type_
            if issubclass(et, C.Structure):
                return [self.field(et, x) for x in v]
            if hasattr(et, "contents"):  # POINTER(struct)[]
                return [self.field(et._type_, x.contents) for x in v]
            return "host:%s[%d]" % (et.__name__, len(v))
        if kind is C.c_void_p:
            return self.ptr(v)
        return float(v) if kind in _FLOATS else int(v)

    def call(self, name, args):
        kinds = hb.SIGNATURES[name][1]
        assert len(args) == len(kinds), "%s takes %d arguments, got %d" % (name, len(kinds), len(args))
        self.calls.append([name, [self.arg(k, v) for k, v in zip(kinds, args)]])
        r = self.ret.get(name, 0)
        return r(self) if callable(r) else r


class _Stub:
    def __init__(self, tr):
        self._tr = tr

    def __getattr__(self, name):
        if not name.startswith("fhvae_"):
            raise AttributeError(name)
        if name == "fhvae_strerror":
            return lambda code: b"stub error"
        return lambda *args: self._tr.call(name, args)


class _Timer:
    on = True

    def __init__(self, tr):
        self._tr = tr

    def start(self):
        self._tr.calls.append(["+"])
        return len(self._tr.calls)

    def stop(self, name, e0):
        self._tr.calls.append(["-", name])


@contextlib.contextmanager
def recording(ret=None):
    tr = Trace(ret)
    words = torch.zeros(4, dtype=torch.int32)
    saved = {n: getattr(hb, n) for n in ("_lib", "_need_gpu", "_stream", "_device_words", "OP_TIMER")}
    state = (dict(hb._DEFER), dict(hb.PAIR_SIDE), dict(hb.LSTM_BWD_REC_HOOK), dict(hb.DISC_BWD_WS), list(hb.LSTM_WORKSPACES),
             os.environ.get("FHVAE_NO_INFER"))
    hb._lib, hb._need_gpu, hb._stream, hb._device_words, hb.OP_TIMER = _Stub(tr), (lambda *ts: None), (lambda: 0), (lambda dev=None: words), _Timer(tr)
    hb._DEFER.update(enabled=True, pending=[], extra=[])
    hb.PAIR_SIDE.update(enabled=True, used=0)
    hb._PAIR_GRAD.clear()
    os.environ.pop("FHVAE_NO_INFER", None)
    torch.manual_seed(0)
    try:
        with _KeepAlive():
            yield tr
    finally:
        for n, v in saved.items():
            setattr(hb, n, v)
        hb._DEFER.clear(); hb._DEFER.update(state[0])
        hb.PAIR_SIDE.update(state[1]); hb.LSTM_BWD_REC_HOOK.update(state[2]); hb.DISC_BWD_WS.update(state[3])
        hb.LSTM_WORKSPACES[:] = state[4]
        hb._PAIR_GRAD.clear()
        os.environ.pop("FHVAE_NO_INFER", None)
        if state[5] is not None:
            os.environ["FHVAE_NO_INFER"] = state[5]


# ---------------------------------------------------------------------------------------------
# tensors
# ---------------------------------------------------------------------------------------------
def f(*shape, grad=False):
    return torch.randn(*shape).requires_grad_(grad)


def bf(*shape):
    return torch.randn(*shape).to(torch.bfloat16)


def i64(*v):
    return torch.tensor(v, dtype=torch.int64)


def i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def u8(n):
    return torch.zeros(n, dtype=torch.uint8)


def sink(tr, *ps):
    for p in ps:
        p._fh_grad = tr.ins(torch.zeros_like(p.detach()))


def bw(tr, outs):
    """Backward from explicit gradients the case holds (registered as inputs)."""
    outs = [o for o in outs if o is not None and o.requires_grad]
    gs = [tr.ins(torch.randn(o.shape)) for o in outs]
    torch.autograd.backward(outs, gs)


CASES = {}


def case(name, **ret):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = (fn, ret)
        return fn
    return deco


# ---------------------------------------------------------------------------------------------
# model ops
# ---------------------------------------------------------------------------------------------
for _relu in (False, True):
    for _sinks in (False, True):
        def _linear(tr, relu=_relu, sinks=_sinks):
            x, w, b = tr.ins(f(3, 4, grad=not sinks), f(5, 4, grad=True), f(5, grad=True))
            if sinks:
                sink(tr, w, b)
            bw(tr, [hb.linear(x, w, b, relu)])
        case("linear relu=%d sinks=%d" % (_relu, _sinks))(_linear)


def _head_params(tr, D, K, sinks):
    ps = tr.ins(f(D, K, grad=True), f(D, grad=True), f(D, K, grad=True), f(D, grad=True))
    if sinks:
        sink(tr, *ps)
    return ps


for _eps in (False, True):
    for _sinks in (False, True):
        def _gh(tr, eps=_eps, sinks=_sinks):
            h = tr.ins(f(3, 6, grad=True))
            e = tr.ins(f(3, 5)) if eps else None
            mu, lv, smp = hb.gauss_head(h, *_head_params(tr, 5, 6, sinks), e)
            assert (smp is None) == (not eps)
            bw(tr, [mu, lv, smp])
        case("gauss_head f32 eps=%d sinks=%d" % (_eps, _sinks))(_gh)

        for _shadows in (False, True):
            for _ok in (0, 1):
                def _ghlp(tr, eps=_eps, sinks=_sinks, shadows=_shadows):
                    h = tr.ins(f(3, 8, grad=True))
                    h_lp = tr.ins(bf(3, 8))
                    e = tr.ins(f(3, 8)) if eps else None
                    sh = tr.ins(bf(16, 8), bf(8, 64)) if shadows else None
                    mu, lv, smp = hb.gauss_head(h, *_head_params(tr, 8, 8, sinks), e, h_lp=h_lp, shadows=sh)
                    bw(tr, [mu, lv, smp])
                    hb.flush_param_grads()
                case("gauss_head bf16 eps=%d sinks=%d shadows=%d desc_ok=%d" % (_eps, _sinks, _shadows, _ok), fhvae_wgrad_desc_ok=_ok)(_ghlp)


@case("gauss_head bf16 only d_mu, wrong-shape shadows")
def _(tr):
    h, h_lp = tr.ins(f(3, 8, grad=True), bf(3, 8))
    mu, lv, smp = hb.gauss_head(h, *_head_params(tr, 8, 8, False), None, h_lp=h_lp, shadows=tr.ins(bf(8, 8), bf(8, 64)))
    bw(tr, [mu])


@case("gauss_head bf16 odd sizes take the f32 head")
def _(tr):
    h, h_lp = tr.ins(f(3, 6, grad=True), bf(3, 6))
    mu, lv, smp = hb.gauss_head(h, *_head_params(tr, 5, 6, False), None, h_lp=h_lp)
    bw(tr, [lv])


def _elbo_args(tr, B=2, T=3, F=8, D=4, time_major=True, grad=True):
    x = tr.ins(f(T, B, F) if time_major else f(B, T, F))
    xs = (F, B * F) if time_major else (T * F, F)
    zs = tr.ins(*[f(B, D, grad=grad) for _ in range(5)])
    return x, xs, zs


for _detach in (False, True):
    for _ns in ("scalar", "tensor"):
        def _elbo(tr, detach=_detach, ns=_ns):
            B, T, F = 2, 3, 8
            x, xs, zs = _elbo_args(tr, time_major=False)
            x_mu, x_lv = tr.ins(f(B * T, F, grad=True), f(B * T, F, grad=True))
            num_segs = tr.ins(i64(5, 7)) if ns == "tensor" else 100.0
            outs = hb.elbo(x, x_mu, x_lv, *zs, num_segs, (B, T, F, xs, (T * F, F)), detach)
            bw(tr, list(outs))
        case("elbo detach=%d num_segs=%s" % (_detach, _ns))(_elbo)

for _side in (False, True):
    for _tm in (False, True):
        def _elbo_pair(tr, side=_side, tm=_tm):
            B, T, F = 2, 3, 8
            hb.PAIR_SIDE["enabled"] = side
            x, xs, zs = _elbo_args(tr, time_major=tm)
            buf = tr.ins(f(T * B, 2 * F, grad=True))
            outs = hb.elbo(x, buf[:, :F], buf[:, F:], *zs, 100.0, (B, T, F, xs, (F, B * F)), False)
            bw(tr, [outs[0]])
        case("elbo pair side=%d time_major=%d" % (_side, _tm))(_elbo_pair)

for _side in (False, True):
    for _sinks in (False, True):
        def _head_elbo(tr, side=_side, sinks=_sinks):
            """The per-frame head behind the lower bound: its backward takes the lower bound's ready-made bf16 operand."""
            B, T, F = 2, 3, 8
            hb.PAIR_SIDE["enabled"] = side
            x, xs, zs = _elbo_args(tr)
            h, h_lp = tr.ins(f(T * B, 8, grad=True), bf(T * B, 8))
            mu, lv, _s = hb.gauss_head(h, *_head_params(tr, F, 8, sinks), None, h_lp=h_lp)
            outs = hb.elbo(x, mu, lv, *zs, 100.0, (B, T, F, xs, (F, B * F)), False)
            bw(tr, [outs[0]])
            assert hb.PAIR_SIDE["used"] == (1 if side else 0)
            hb.flush_param_grads()
        case("head + elbo pair side=%d sinks=%d" % (_side, _sinks), fhvae_wgrad_desc_ok=1, fhvae_elbo_colsum_rows=3)(_head_elbo)


for _qy in (False, True):
    def _loss(tr, qy=_qy):
        lb, q = tr.ins(f(4, grad=True), f((), grad=qy))
        bw(tr, [hb.fused_loss(lb, q, 10.0)])
    case("fused_loss qy_grad=%d" % _qy)(_loss)

for _sinks in (False, True):
    def _gather(tr, sinks=_sinks):
        table, idx = tr.ins(f(6, 4, grad=True), i64(1, 5, 1))
        if sinks:
            sink(tr, table)
        bw(tr, [hb.mu2_gather(table, idx)])
    case("mu2_gather sinks=%d" % _sinks)(_gather)


@case("raw_gather_rows / raw_scatter_rows_ with a shard offset")
def _(tr):
    table, idx, rows = tr.ins(f(6, 4), i64(7, 9), f(2, 4))
    hb.raw_gather_rows(table, idx, 6)
    hb.raw_scatter_rows_(table, rows, idx, 6, 0.5)


# ---------------------------------------------------------------------------------------------
# LSTM
# ---------------------------------------------------------------------------------------------
def _lstm_args(tr, xmode, dtype, head, L=2, H=8, B=2, T=3, I=4, Ic=3, grad=True, sinks=False):
    x = tr.ins(f(T, B, I)) if xmode in ("x", "both") else None
    if x is not None and dtype == hb.BF16:
        x._fh_lp = tr.ins(bf(T, B, I))
    xc = tr.ins(f(B, Ic, grad=grad)) if xmode in ("xc", "both") else None
    params = []
    for l in range(L):
        nin = H if l else (I if x is not None else 0) + (Ic if xc is not None else 0)
        params += tr.ins(f(4 * H, nin, grad=grad), f(4 * H, H, grad=grad), f(4 * H, grad=grad), f(4 * H, grad=grad))
    if sinks:
        sink(tr, *params)
    hd = tr.ins(f(8, 16, grad=grad), f(8, 16, grad=grad)) if head else None
    return x, xc, T, params, dtype, hd


def _check_tags(out, hn, dtype, top, head):
    bf16 = dtype == hb.BF16
    assert (getattr(hn, "_fh_lp", None) is not None) == (bf16 and top == 0)
    assert (hn._fh_head is not None) == (bf16 and head)
    if out is not None and out.dim() == 3:
        assert (getattr(out, "_fh_lp", None) is not None) == bf16 and (out._fh_head is not None) == (bf16 and head)


_RET_LSTM = dict(fhvae_lstm_lp_bytes=96, fhvae_lstm_pre_elems=7, fhvae_lstm_form=1, fhvae_lstm_layout_id=18)
for _dt in (hb.F32, hb.BF16):
    for _top in (0, 1, 2):
        for _xm in ("x", "xc", "both"):
            for _head in (False, True):
                _nm = "dtype=%d top=%d %s head=%d" % (_dt, _top, _xm, _head)

                def _fwd_bwd(tr, dt=_dt, top=_top, xm=_xm, head=_head):
                    x, xc, T, params, dtype, hd = _lstm_args(tr, xm, dt, head, L=1)
                    out, hn = hb.lstm_seq(x, xc, T, params, dtype, top, hd)
                    _check_tags(out, hn, dtype, top, head)
                    assert hb.LAST_LSTM_FORM == {"form": 1, "layout": 18}
                    bw(tr, [out, hn])
                case("lstm_seq " + _nm, **_RET_LSTM)(_fwd_bwd)

                def _infer(tr, dt=_dt, top=_top, xm=_xm, head=_head):
                    x, xc, T, params, dtype, hd = _lstm_args(tr, xm, dt, head, L=1)
                    out, hn = hb.lstm_seq_infer(x, xc, T, params, dtype, top, hd)
                    assert (out is None) == (top == 0 and dt == hb.BF16) and not hn.requires_grad
                    _check_tags(out, hn, dtype, top, head)
                case("lstm_seq_infer " + _nm, fhvae_lstm_infer_cs_elems=(5 if _head else 0), **_RET_LSTM)(_infer)


@case("lstm_seq with every library query answering 0")
def _(tr):
    x, xc, T, params, dtype, hd = _lstm_args(tr, "both", hb.BF16, True, L=1)
    out, hn = hb.lstm_seq(x, xc, T, params, dtype, 2, hd)
    bw(tr, [out, hn])
    hb.lstm_seq_infer(x, xc, T, params, dtype, 2, hd)


for _which in ("out", "hn"):
    def _one_grad(tr, which=_which):
        x, xc, T, params, dtype, hd = _lstm_args(tr, "both", hb.BF16, False)
        out, hn = hb.lstm_seq(x, xc, T, params, dtype, 2, hd)
        bw(tr, [out if which == "out" else hn])
    case("lstm_seq backward with a gradient for %s only" % _which, fhvae_lstm_ws_below_elems=11, **_RET_LSTM)(_one_grad)


@case("lstm_seq backward: no gradient wanted for xc", **_RET_LSTM)
def _(tr):
    x, xc, T, params, dtype, hd = _lstm_args(tr, "xc", hb.F32, False, L=1)
    xc.requires_grad_(False)
    out, hn = hb.lstm_seq(x, xc, T, params, dtype, 2, hd)
    bw(tr, [out, hn])


def _three_nets(tr, dtype=hb.BF16):
    nets = [_lstm_args(tr, xm, dtype, False, L=1 + (k == 2), sinks=True) for k, xm in enumerate(("x", "both", "xc"))]
    return [hb.lstm_seq(*a[:4], a[4], 2, a[5]) for a in nets]


@case("lstm_seq deferred backward: three nets, one flush", **_RET_LSTM)
def _(tr):
    outs = _three_nets(tr)
    for out, hn in outs:
        bw(tr, [out, hn])
    assert len(hb._DEFER["pending"]) == 3 and tr.n_calls() and all(c[0] != "fhvae_lstm_param_grads_multi" for c in tr.calls)
    hb.flush_param_grads()
    assert not hb._DEFER["pending"]
    hb.flush_param_grads()  # nothing queued: no call


@case("lstm_seq deferred backward: flush_param_grads_except_last, then the rest", fhvae_lstm_ws_below_elems=11, **_RET_LSTM)
def _(tr):
    outs = _three_nets(tr, hb.F32)
    bw(tr, list(outs[0]))
    hb.flush_param_grads_except_last()  # one queued: no call
    bw(tr, list(outs[1]))
    bw(tr, list(outs[2]))
    hb.flush_param_grads_except_last()
    assert len(hb._DEFER["pending"]) == 1
    hb.set_defer_param_grads(False)  # flushes
    assert not hb._DEFER["pending"] and not hb._DEFER["enabled"]


@case("lstm_seq deferred backward with LSTM_BWD_REC_HOOK", **_RET_LSTM)
def _(tr):
    fired = []
    hb.LSTM_BWD_REC_HOOK["fn"] = lambda sinks: (fired.append(len(sinks)), tr.calls.append(["<hook>", [len(sinks)]]), hb.flush_param_grads_except_last())
    for out, hn in _three_nets(tr):
        bw(tr, [out, hn])
    assert fired == [4, 4, 8]
    hb.flush_param_grads()


for _sinks in (False, True):
    def _hook_plain(tr, sinks=_sinks):
        hb.set_defer_param_grads(False)
        hb.LSTM_BWD_REC_HOOK["fn"] = lambda s: tr.calls.append(["<hook>", [len(s)]])
        x, xc, T, params, dtype, hd = _lstm_args(tr, "both", hb.BF16, True, sinks=sinks)
        out, hn = hb.lstm_seq(x, xc, T, params, dtype, 1, hd)
        bw(tr, [out, hn])
        assert not hb._DEFER["pending"]
    case("lstm_seq backward with LSTM_BWD_REC_HOOK, not deferred, sinks=%d" % _sinks, **_RET_LSTM)(_hook_plain)


@case("lstm_seq backward with sinks, deferral off: one call", **_RET_LSTM)
def _(tr):
    hb.set_defer_param_grads(False)
    x, xc, T, params, dtype, hd = _lstm_args(tr, "x", hb.F32, False, sinks=True)
    out, hn = hb.lstm_seq(x, xc, T, params, dtype, 2, hd)
    bw(tr, [out, hn])
    assert all(p.grad is None for p in params)


@case("lstm_seq backward with sinks on some parameters only: not deferred", **_RET_LSTM)
def _(tr):
    x, xc, T, params, dtype, hd = _lstm_args(tr, "x", hb.F32, False, L=1)
    sink(tr, params[0], params[2])
    out, hn = hb.lstm_seq(x, xc, T, params, dtype, 2, hd)
    bw(tr, [out, hn])
    assert not hb._DEFER["pending"] and params[0].grad is None and params[1].grad is not None


for _env in (False, True):
    for _dt in (hb.F32, hb.BF16):
        def _eval(tr, env=_env, dt=_dt):
            if env:
                os.environ["FHVAE_NO_INFER"] = "1"
            assert hb.infer_enabled() == (not env)
            x, xc, T, params, dtype, hd = _lstm_args(tr, "x", dt, False, grad=False)
            out, hn = hb.lstm_seq_eval(x, xc, T, params, dtype, 0, hd)
            assert (out is None) == (dt == hb.BF16)
        case("lstm_seq_eval FHVAE_NO_INFER=%d dtype=%d" % (_env, _dt), **_RET_LSTM)(_eval)


@case("cast_bf16 / to_time_major")
def _(tr):
    t, x = tr.ins(f(3, 5), f(2, 3, 4))
    hb.cast_bf16(t)
    assert not hasattr(hb.to_time_major(x), "_fh_lp")
    assert hb.to_time_major(x, with_bf16=True)._fh_lp.dtype == torch.bfloat16


# ---------------------------------------------------------------------------------------------
# discriminative loss, shards, contractions, optimizer, sampler
# ---------------------------------------------------------------------------------------------
for _lp in (False, True):
    for _sinks in (False, True):
        def _disc(tr, lp=_lp, sinks=_sinks):
            q, table, idx = tr.ins(f(3, 4, grad=True), f(6, 4, grad=True), i64(0, 5, 2))
            if sinks:
                sink(tr, table)
            bw(tr, [hb.disc_lse(q, table, idx, lp=lp, sign=-1.0)])
        case("disc_lse lp=%d sinks=%d" % (_lp, _sinks), fhvae_disc_lse_ws_bytes=40, fhvae_disc_lse_bwd_ws_bytes=64)(_disc)


@case("raw_disc_fwd / raw_disc_bwd options", fhvae_disc_lse_bwd_ws_bytes=64)
def _(tr):
    q, table, idx, out3, dts, g = tr.ins(f(3, 4), f(6, 4), i64(0, 5, 2), f(3, 3), f(6, 4), f(1))
    rmax, rsum, tgt, ce = hb.raw_disc_fwd(q, table, idx, row0=6, want_ce=False, out3=out3)
    assert ce is None and rmax.data_ptr() == out3.data_ptr()
    hb.raw_disc_fwd(q, table, idx, lp=True, ce_scale=-1.0)
    assert hb.raw_disc_bwd(q, table, idx, rmax, rsum, g, 0.25, row0=6, dt_sink=dts)[1] is None
    hb.raw_disc_bwd(q, table, idx, rmax, rsum, g, 0.25, ws_bytes=0)
    hb.raw_disc_bwd(q, table, idx, rmax, rsum, g, 0.25, ws_bytes=32, lp=True)
    hb.raw_disc_bwd(q, table, idx, rmax, rsum, g, 0.25, need_dq=False)
    hb.raw_disc_bwd(q, table, idx, rmax, rsum, g, 0.25, need_dt=False)
    hb.DISC_BWD_WS["bytes"] = 0
    hb.raw_disc_bwd(q, table, idx, rmax, rsum, g, 0.25)


@case("shard packers, disc_merge_partials, raw_disc_ce_mean")
def _(tr):
    q, idx, parts, dq, dm = tr.ins(f(3, 4), i64(0, 5, 2), f(2, 3, 5), f(5, 4), f(2, 4))
    pk = hb.shard_pack(q, idx)
    hb.shard_unpack(pk)
    m, s, t = hb.disc_merge_partials(parts)
    hb.raw_disc_ce_mean(m, s, t, -1.0)
    buf = hb.shard_bwd_pack(dq, 0.5, dm, 1, 5, 4)
    hb.shard_bwd_pack(None, 1.0, dm, 1, 5, 4)
    hb.shard_bwd_pack(dq, 1.0, None, 0, 5, 4)
    hb.shard_bwd_unpack(buf, 1, 2)
    hb.shard_bwd_unpack(buf, 1, 2, want_dq=False)
    hb.shard_bwd_unpack(buf, 1, 2, want_dmu2=False)


@case("wgrad_bf16_ / wgrad_f32_ / proj_bf16")
def _(tr):
    c, a, b, a32, b32, w, bias, out = tr.ins(f(4, 6), bf(5, 4), bf(5, 8)[:, :6], f(5, 4), f(5, 6), bf(3, 4), f(3), f(5, 8))
    assert hb.wgrad_bf16_(c, a, b) is c and hb.wgrad_f32_(c, a32, b32) is c
    hb.proj_bf16(a, w)
    assert hb.proj_bf16(a, w, bias, out[:, :3]).data_ptr() == out.data_ptr()


@case("adam_step_")
def _(tr):
    p, g, m, v, p_lp = tr.ins(f(10), f(10), f(10), f(10), bf(10))
    step, buf = tr.ins(i32(3), torch.zeros(hb.ADAM_STEP_WORDS, dtype=torch.int32))
    for flags, sd in ((0, step), (hb.ADAM_ZERO_GRAD, step), (hb.ADAM_ADVANCE, buf), (hb.ADAM_ZERO_GRAD | hb.ADAM_ADVANCE, buf)):
        hb.adam_step_(p, g, m, v, sd, 1e-3, 0.95, 0.999, 1e-8, flags=flags)
    hb.adam_step_(p, g, m, v, step, 1e-3, 0.95, 0.999, 1e-8, grad_scale=0.5, p_lp=p_lp)
    n = tr.n_calls()
    e = torch.empty(0)
    hb.adam_step_(e, e, e, e, step, 1e-3, 0.95, 0.999, 1e-8)  # an empty shard: no call
    assert tr.n_calls() == n


@case("segment_gather")
def _(tr):
    pool, start, mean, inv = tr.ins(f(20, 4), i64(0, 7), f(4), f(4))
    assert hb.segment_gather(pool, start, 3).shape == (2, 3, 4)
    assert hb.segment_gather(pool, start, 3, mean, inv, time_major=True)[1].shape == (3, 2, 4)


@case("Mu2Estimator")
def _(tr):
    est = hb.Mu2Estimator(6, 4, "cpu")
    tr.ins(est.zsum, est.count)
    est.add(*tr.ins(f(3, 4, grad=True), i64(0, 5, 2)))
    mu2, count = est.result(0.5)
    assert count is est.count and mu2.shape == (6, 4)


@case("SortedMu2Estimator, mu2_load_table")
def _(tr):
    est = hb.SortedMu2Estimator(6, 4, "cpu")
    tr.ins(est.zsum, est.count, est.status)
    est.add(*tr.ins(f(3, 4, grad=True), i64(0, 2, 5)))
    n = tr.n_calls()
    est.add(f(0, 4), i64())  # no rows: no call
    assert tr.n_calls() == n
    est.check()
    mu2, count = est.result(0.5)
    assert count is est.count and mu2.shape == (6, 4)
    est.load_into(*tr.ins(f(6, 4), f(6, 4), f(6, 4)), 0.5)
    assert hb.SortedMu2Estimator(6, 4, "cpu", status=est.status).status is est.status
    est.status.fill_(hb.HS_CAP | hb.HS_UNSORTED)
    with pytest.raises(RuntimeError, match="segment total above capacity, local indices not sorted"):
        est.check()


# ---------------------------------------------------------------------------------------------
# data ops: one builder of good arguments per wrapper (the refusals below bend one argument each)
# ---------------------------------------------------------------------------------------------
def g_hs_select():
    return dict(seq_ptr=i64(0, 2, 3, 6, 9), block_seqs=i64(1, 3), seg_ids=i64(*range(6)), local_idx=i64(*range(6)), n_out=i64(0), status=i32(0))


def g_feats(ftype="fbank"):
    return dict(wave=f(40), wave_ptr=i64(0, 20, 40), frame_ptr=i64(0, 2, 4), dft_basis=f(32, 16), mel_basis=f(16, 16) if ftype == "fbank" else None,
                n_fft=16, hop=4, n_mels=4, ftype=ftype, out=f(4, 4 if ftype == "fbank" else 9), status=i32(0))


def g_kaldi_fbank(dither=0.0):
    return dict(wave=f(40), wave_ptr=i64(0, 20, 40), frame_ptr=i64(0, 2, 4), stream_ids=i64(11, 12) if dither else None, dft_basis=f(32, 16),
                mel_basis=f(16, 16), frame_len=10, frame_shift=5, padded_len=16, n_mels=4, preemph=0.97, dither=dither, seed=-3,
                flags=hb.KALDI_REMOVE_DC | hb.KALDI_USE_LOG, out=f(4, 4), status=i32(0))


def g_kaldi_cm():
    return dict(payload=u8(48), desc=u8(2 * hb.KALDI_CM_DESC.itemsize), n_tiles=2, mat=f(5, 3), status=i32(0))


def _decompress(payload, desc, n_tiles, mat, status):
    return hb.kaldi_decompress(payload, desc, n_tiles, mat, status)


def _compress(payload, desc, n_tiles, mat, status):
    return hb.kaldi_compress(mat, desc, n_tiles, payload, status)


def g_flac_scan():
    return dict(buf=u8(24), desc=u8(2 * hb.FLAC_DESC.itemsize), info=torch.zeros(24, dtype=torch.int32))


def g_flac_decode(out=True):
    return dict(buf=u8(24), desc=u8(2 * hb.FLAC_DESC.itemsize), cand_pos=i64(0, 9, 15), cand_status=i32(0, 0, 0), cand_end=i64(0, 0, 0),
                cand_spos=i64(0, 0, 0), out=torch.zeros(30, dtype=torch.int32) if out else None)


def g_resample(exc=False):
    return dict(wave_in=f(40), in_ptr=i64(0, 20, 40), out_ptr=i64(0, 10, 20), row_ptr=i64(0, 1, 2), n_rows=2, bank=f(16, 32), chunks=torch.zeros(1, 2, dtype=torch.int32),
                L=16, M=32, P=1, WL=9, ratio=0.5, exc=u8(5) if exc else None, alt=f(7) if exc else None, alt_wl=3, wave_out=f(20), status=i32(0))


def g_istft():
    return dict(spec=f(4, 9, 2), wave_ptr=i64(0, 4, 8), frame_ptr=i64(0, 2, 4), synth_basis=f(16, 32), win_sq=f(16), n_fft=16, hop=4, frames_ws=f(4, 16),
                wave_out=f(8), status=i32(0))


def g_project(full=True):
    return dict(wave=f(8), wave_ptr=i64(0, 4, 8), frame_ptr=i64(0, 2, 4), dft_basis=f(32, 16), mag=f(4, 9), tprev=f(4, 9, 2) if full else None, coef=0.99,
                n_fft=16, hop=4, rebuilt=f(4, 9, 2) if full else None, nxt=f(4, 9, 2), status=i32(0))


def g_deemph():
    return dict(wave=f(8), wave_ptr=i64(0, 4, 8), coef=0.97, out=f(8), status=i32(0))


def g_mel_invert():
    return dict(mel=f(3, 4), bin_filt=i32(*range(9)), bin_w=f(9, 2), filt_first=i32(0, 2, 4, 6), filt_off=i32(0, 2, 4, 6, 8), filt_w=f(8), inv_l=0.5,
                beta=f(5), out=f(3, 9), status=i32(0))


def g_sv_hist(D=16):
    return dict(emb=f(5, D), label=i32(0, 1, 0, -1, 1), n_bins=64)


def g_tsne_affinity(D=16):
    return dict(x=f(10, D), perplexity=2.0)


def g_tsne_step():
    return dict(x=f(10, 16), beta=f(10), m=f(10), z=f(10), y=f(10, 2), v=f(10, 2), g=f(10, 2), exaggeration=12.0, momentum=0.5, lr=200.0)


def g_tsne_grad():
    return dict(x=f(10, 16), beta=f(10), m=f(10), z=f(10), y=f(10, 2))


def g_acc_sorted():
    return dict(z2_mu=f(3, 4), local_idx=i64(0, 2, 5), zsum=f(6, 4), count=f(6), status=i32(0))


def g_load_table():
    return dict(zsum=f(6, 4), count=f(6), table=f(6, 4), m_rows=f(6, 4), v_rows=f(6, 4), ratio=0.5)


def g_pack_partials():
    return dict(zsum=f(6, 4), count=f(6), out=f(6, 5))


def g_merge_shard():
    return dict(parts=f(2, 6, 5), row0=1, row1=4, shard=f(3, 4), m_rows=f(3, 4), v_rows=f(3, 4), ratio=0.5)


def g_adam():
    return dict(p=f(10), g=f(10), m=f(10), v=f(10), step_dev=i32(3), lr=1e-3, beta1=0.95, beta2=0.999, eps=1e-8)


def _good(name, fn, make, **ret):
    def run(tr):
        kw = make()
        tr.ins(*[v for v in kw.values() if isinstance(v, torch.Tensor)])
        fn(**kw)
    case(name, **ret)(run)


_good("hs_select", hb.hs_select, g_hs_select)
_good("feats_fwd fbank", hb.feats_fwd, g_feats)
_good("feats_fwd spec", hb.feats_fwd, lambda: g_feats("spec"))
_good("kaldi_fbank_fwd", hb.kaldi_fbank_fwd, g_kaldi_fbank)
_good("kaldi_fbank_fwd dither", hb.kaldi_fbank_fwd, lambda: g_kaldi_fbank(1.0))
_good("kaldi_decompress", _decompress, g_kaldi_cm)
_good("kaldi_compress", _compress, g_kaldi_cm)
_good("flac_scan", hb.flac_scan, g_flac_scan)
_good("flac_decode", hb.flac_decode, g_flac_decode)
_good("flac_decode verify only", hb.flac_decode, lambda: g_flac_decode(False))
_good("resample_fwd", hb.resample_fwd, g_resample)
_good("resample_fwd with exceptions", hb.resample_fwd, lambda: g_resample(True))
_good("synth_istft", hb.synth_istft, g_istft)
_good("synth_project", hb.synth_project, g_project)
_good("synth_project first iteration", hb.synth_project, lambda: g_project(False))
_good("synth_deemph", hb.synth_deemph, g_deemph)
_good("mel_invert", hb.mel_invert, g_mel_invert)
_good("mel_invert linear in and out", lambda **kw: hb.mel_invert(in_log=False, out_log=False, **kw), g_mel_invert)
_good("sv_hist rows read in place", hb.sv_hist, g_sv_hist, fhvae_sv_hist_ws_bytes=24)
_good("sv_hist padded rows", hb.sv_hist, lambda: g_sv_hist(5), fhvae_sv_hist_ws_bytes=24)
_good("tsne_affinity", hb.tsne_affinity, g_tsne_affinity, fhvae_tsne_ws_bytes=24)
_good("tsne_affinity padded rows", hb.tsne_affinity, lambda: g_tsne_affinity(5), fhvae_tsne_ws_bytes=24)
_good("tsne_step", hb.tsne_step, g_tsne_step, fhvae_tsne_ws_bytes=24)
_good("tsne_grad", hb.tsne_grad, g_tsne_grad, fhvae_tsne_ws_bytes=24)
_good("mu2_accumulate_sorted", hb.mu2_accumulate_sorted, g_acc_sorted)
_good("mu2_load_table", hb.mu2_load_table, g_load_table)
_good("hs_pack_partials", hb.hs_pack_partials, g_pack_partials)
_good("mu2_merge_load_shard", hb.mu2_merge_load_shard, g_merge_shard)


@case("tsne with the caller's workspace and kl", fhvae_tsne_ws_bytes=24)
def _(tr):
    kw = g_tsne_step()
    tr.ins(*[v for v in kw.values() if isinstance(v, torch.Tensor)])
    ws = hb.tsne_workspace(kw["x"])
    assert ws.numel() == 24
    kl = tr.ins(f(1))
    hb.tsne_affinity(kw["x"], 2.0, ws=ws)
    torch.Tensor.is_cuda = property(lambda t: True)  # (kl's own device check, beside _need_gpu)
    try:
        hb.tsne_step(kl=kl, ws=ws, **kw)
    finally:
        del torch.Tensor.is_cuda
    hb.tsne_grad(kw["x"], kw["beta"], kw["m"], kw["z"], kw["y"], exaggeration=4.0, ws=ws)


@case("mu2_merge_load_shard empty shard: no call")
def _(tr):
    kw = dict(g_merge_shard(), row0=2, row1=2, shard=f(0, 4), m_rows=f(0, 4), v_rows=f(0, 4))
    hb.mu2_merge_load_shard(**kw)
    assert tr.n_calls() == 0


@case("cell_trace / cell_trace_collect", fhvae_trace_collect=0)
def _(tr):
    hb.cell_trace(True)
    assert hb.cell_trace_collect(cap=8) == {}


@case("a failing call names its symbol", fhvae_cast_bf16=7)
def _(tr):
    with pytest.raises(RuntimeError, match=r"fhvae_cast_bf16 failed: stub error \(code 7\)"):
        hb.cast_bf16(tr.ins(f(2, 3)))


# ---------------------------------------------------------------------------------------------
# refusals: (name, wrapper, good arguments, what to bend, what the message must name).  Each must raise RuntimeError before
# any C call.
# ---------------------------------------------------------------------------------------------
REFUSALS = []


def refuse(fn, make, who, **bends):
    """One refusal per keyword: `arg=new value` or `arg=callable(good arguments) -> new value` (`arg__1`, `arg__2`: more
    values for the same argument)."""
    for k, v in bends.items():
        name = "%s: %s" % (who, k)
        n = sum(1 for r in REFUSALS if r[0].split(" #")[0] == name)
        REFUSALS.append((name + (" #%d" % n if n else ""), fn, make, k.split("__")[0], v, who))


def nc(t):
    """The same values, not contiguous."""
    return torch.stack([t, t], dim=-1)[..., 0]


f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731

refuse(hb.hs_select, g_hs_select, "hs_select", seq_ptr=i32(0, 2, 3, 6, 9), block_seqs=lambda a: nc(a["block_seqs"]), n_out=i32(0), status=i64(0),
       local_idx=i64(0, 1, 2), seg_ids=lambda a: nc(a["seg_ids"]))
for _ft in ("fbank", "spec"):
    refuse(hb.feats_fwd, lambda ft=_ft: g_feats(ft), "feats_fwd", wave=f64(40), dft_basis=lambda a: nc(a["dft_basis"]), out=lambda a: nc(a["out"]),
           wave_ptr=i32(0, 20, 40), frame_ptr=lambda a: nc(a["frame_ptr"]), status=i64(0), frame_ptr__1=i64(0, 2), out__1=f(4), dft_basis__1=f(32, 32),
           out__2=f(4, 5), n_fft=32)
refuse(hb.feats_fwd, g_feats, "feats_fwd", mel_basis=None, mel_basis__1=f(16, 32), mel_basis__2=f64(16, 16), n_mels=20)
for _di in (0.0, 1.0):
    refuse(hb.kaldi_fbank_fwd, lambda di=_di: g_kaldi_fbank(di), "kaldi_fbank_fwd", wave=f64(40), mel_basis=lambda a: nc(a["mel_basis"]), out=f64(4, 4),
           wave_ptr=i32(0, 20, 40), frame_ptr=lambda a: nc(a["frame_ptr"]), status=i64(0), status__1=i32(0, 0), frame_ptr__1=i64(0, 2), out__1=f(4),
           dft_basis=f(32, 32), mel_basis__1=f(16, 32), out__2=f(4, 5), padded_len=64, n_mels=20)
refuse(hb.kaldi_fbank_fwd, lambda: g_kaldi_fbank(1.0), "kaldi_fbank_fwd", stream_ids=None, stream_ids__1=i64(1, 2, 3), stream_ids__2=i32(1, 2))
for _fn, _who in ((_decompress, "kaldi_decompress"), (_compress, "kaldi_compress")):
    refuse(_fn, g_kaldi_cm, _who, payload=torch.zeros(48, dtype=torch.int8), payload__1=u8(48).view(4, 12), payload__2=lambda a: nc(a["payload"]), payload__3=u8(46),
           desc=torch.zeros(80, dtype=torch.int8), desc__1=lambda a: nc(a["desc"]), desc__2=u8(0), desc__3=u8(60), mat=f64(5, 3), mat__1=f(15), mat__2=lambda a: nc(a["mat"]),
           status=i64(0), status__1=i32(0, 0))
for _fn, _mk, _who in ((hb.flac_scan, g_flac_scan, "flac_scan"), (hb.flac_decode, g_flac_decode, "flac_decode")):
    refuse(_fn, _mk, _who, buf=torch.zeros(24, dtype=torch.int8), buf__1=u8(24).view(2, 12), buf__2=lambda a: nc(a["buf"]), buf__3=u8(0),
           desc=torch.zeros(96, dtype=torch.int8), desc__1=lambda a: nc(a["desc"]), desc__2=u8(0), desc__3=u8(50))
refuse(hb.flac_scan, g_flac_scan, "flac_scan", info=torch.zeros(24, dtype=torch.int64), info__1=torch.zeros(23, dtype=torch.int32), info__2=lambda a: nc(a["info"]))
for _o in (True, False):
    refuse(hb.flac_decode, lambda o=_o: g_flac_decode(o), "flac_decode", cand_pos=i32(0, 9, 15), cand_status=i64(0, 0, 0), cand_end=i64(0, 0), cand_spos=lambda a: nc(a["cand_spos"]))
refuse(hb.flac_decode, g_flac_decode, "flac_decode", out=torch.zeros(30, dtype=torch.int64), out__1=torch.zeros(5, 6, dtype=torch.int32), out__2=lambda a: nc(a["out"]))
for _e in (False, True):
    refuse(hb.resample_fwd, lambda e=_e: g_resample(e), "resample_fwd", wave_in=f64(40), bank=lambda a: nc(a["bank"]), wave_out=f64(20), in_ptr=i32(0, 20, 40),
           out_ptr=lambda a: nc(a["out_ptr"]), row_ptr=i64(0, 1, 2).view(1, 3), row_ptr__1=i64(0, 1), status=i64(0), status__1=i32(0, 0), wave_in__1=f(2, 20),
           wave_out__1=f(2, 10), bank__1=f(16), bank__2=f(32, 32), bank__3=f(16, 24), chunks=torch.zeros(1, 2, dtype=torch.int64), chunks__1=torch.zeros(2, 2, dtype=torch.int32),
           chunks__2=lambda a: nc(a["chunks"]), P=3)
refuse(hb.resample_fwd, g_resample, "resample_fwd", exc=u8(5), alt=f(7), in_ptr=i64(0), out_ptr=i64(0), row_ptr=i64(0))
refuse(hb.resample_fwd, lambda: g_resample(True), "resample_fwd", exc=None, alt=None, alt__1=f64(7), exc__1=torch.zeros(5, dtype=torch.int8), exc__2=u8(6).view(2, 3), exc__3=lambda a: nc(a["exc"]))
refuse(hb.synth_istft, g_istft, "synth_istft", spec=f64(4, 9, 2), wave_out=lambda a: nc(a["wave_out"]), wave_ptr=i32(0, 4, 8), frame_ptr=i64(0, 2), frame_ptr__1=lambda a: nc(a["frame_ptr"]),
       frame_ptr__2=i64(0, 2, 4).view(1, 3), status=i64(0), status__1=i32(0, 0), spec__1=f(4, 18), spec__2=f(4, 8, 2), synth_basis=f(16, 16), win_sq=f(15), frames_ws=f(3, 16),
       wave_out__1=f(2, 4), n_fft=32)
for _full in (True, False):
    refuse(hb.synth_project, lambda fu=_full: g_project(fu), "synth_project", wave=f64(8), nxt=lambda a: nc(a["nxt"]), wave_ptr=i32(0, 4, 8), frame_ptr=i64(0, 2),
           status=i64(0), status__1=i32(0, 0), dft_basis=f(32, 32), mag=f(36), mag__1=f(4, 8), wave__1=f(2, 4), nxt__1=f(4, 9), n_fft=32)
refuse(hb.synth_project, g_project, "synth_project", tprev=f(3, 9, 2), rebuilt=f(4, 9, 3), tprev__1=f64(4, 9, 2))
refuse(hb.synth_deemph, g_deemph, "synth_deemph", wave=f64(8), out=lambda a: nc(a["out"]), wave_ptr=i32(0, 4, 8), wave_ptr__1=i64(0), status=i64(0), status__1=i32(0, 0),
       wave__1=f(2, 4), out__1=f(9))
refuse(hb.mel_invert, g_mel_invert, "mel_invert", mel=f64(3, 4), bin_w=lambda a: nc(a["bin_w"]), filt_w=f64(8), beta=f64(5), out=lambda a: nc(a["out"]),
       bin_filt=i64(*range(9)), filt_first=lambda a: nc(a["filt_first"]), filt_off=i32(0, 2, 4, 6, 8).view(1, 5), status=i64(0), status__1=i32(0, 0), mel__1=f(12), out__1=f(27),
       out__2=f(4, 9), bin_filt__1=i32(*range(8)), bin_w__1=f(9, 3), filt_first__1=i32(0, 2, 4), filt_off__1=i32(0, 2, 4, 6), filt_w__1=f(4, 2), beta__1=f(5, 1), beta__2=f(0))
for _D in (16, 5):
    refuse(hb.sv_hist, lambda D=_D: g_sv_hist(D), "sv_hist", emb=f64(5, 16), emb__1=f(5), label=i64(0, 1, 0, -1, 1), label__1=i32(0, 1, 0, 1).view(2, 2), label__2=i32(0, 1, 0),
           emb__2=f(0, 16), emb__3=f(5, 0), emb__4=f(5, 129), n_bins=32, n_bins__1=16384, n_bins__2=96)
for _fn, _mk, _who in ((hb.tsne_workspace, lambda: dict(x=f(10, 16)), "tsne_workspace"), (hb.tsne_affinity, g_tsne_affinity, "tsne_affinity"),
                       (hb.tsne_step, g_tsne_step, "tsne_step"), (hb.tsne_grad, g_tsne_grad, "tsne_grad")):
    refuse(_fn, _mk, _who, x=f64(10, 16), x__1=f(160), x__2=f(7, 16), x__3=f(10, 0), x__4=f(10, 129))
refuse(hb.sv_hist, lambda: dict(emb=f(0, 16), label=i32(), n_bins=64), "sv_hist", n_bins=64)  # (no rows at all)
refuse(hb.tsne_affinity, g_tsne_affinity, "tsne_affinity", perplexity=0.5, perplexity__1=3.5, perplexity__2=float("nan"))
refuse(hb.tsne_step, g_tsne_step, "tsne_step: beta", beta=f64(10), beta__1=f(9), beta__2=lambda a: nc(a["beta"]), beta__3=f(10, 1))
refuse(hb.tsne_step, g_tsne_step, "tsne_step: m", m=f(9))
refuse(hb.tsne_step, g_tsne_step, "tsne_step: z", z=f(9))
refuse(hb.tsne_step, g_tsne_step, "tsne_step: y", y=f(10), y__1=f64(10, 2), y__2=lambda a: nc(a["y"]))
refuse(hb.tsne_step, g_tsne_step, "tsne_step: v", v=f(10, 3))
refuse(hb.tsne_step, g_tsne_step, "tsne_step: g", g=f(9, 2))
refuse(lambda **kw: hb.tsne_step(**kw), lambda: dict(g_tsne_step(), kl=f(1)), "tsne_step: kl", kl=f(1), kl__1=f64(1), kl__2=f(2))  # (a CPU kl is refused by the wrapper itself)
refuse(hb.tsne_grad, g_tsne_grad, "tsne_grad: beta", beta=f(9))
refuse(hb.tsne_grad, g_tsne_grad, "tsne_grad: m", m=f64(10))
refuse(hb.tsne_grad, g_tsne_grad, "tsne_grad: z", z=lambda a: nc(a["z"]))
refuse(hb.tsne_grad, g_tsne_grad, "tsne_grad: y", y=f(10, 3))
refuse(hb.mu2_accumulate_sorted, g_acc_sorted, "mu2_accumulate_sorted", local_idx=i32(0, 2, 5), local_idx__1=lambda a: nc(a["local_idx"]), status=i64(0), local_idx__2=i64(0, 2),
       zsum=f(6, 5), count=f(5))
refuse(hb.mu2_load_table, g_load_table, "mu2_load_table", zsum=f64(6, 4), table=lambda a: nc(a["table"]), m_rows=f(6, 3), v_rows=f(5, 4), count=f(5), count__1=f64(6))
refuse(hb.hs_pack_partials, g_pack_partials, "hs_pack_partials", zsum=f64(6, 4), zsum__1=lambda a: nc(a["zsum"]), count=f(5), out=f(6, 4), out__1=f64(6, 5))
refuse(hb.mu2_merge_load_shard, g_merge_shard, "mu2_merge_load_shard", parts=f64(2, 6, 5), parts__1=lambda a: nc(a["parts"]), row0=-1, row0__1=5, row1=7, shard=f64(3, 4),
       m_rows=lambda a: nc(a["m_rows"]), v_rows=f(2, 4))
refuse(hb.adam_step_, g_adam, "adam_step_", g=f64(10), m=lambda a: nc(a["m"]), v=f(9), p=f(11), p_lp=f(10), p_lp__1=bf(9), p_lp__2=lambda a: nc(bf(10)), step_dev=i64(3))
refuse(lambda **kw: hb.adam_step_(flags=hb.ADAM_ADVANCE, **kw), g_adam, "ADAM_ADVANCE", step_dev=i32(3))


def _run_case(name):
    fn, ret = CASES[name]
    with recording(ret) as tr:
        fn(tr)
    return tr.calls


def _run_refusal(r):
    name, fn, make, key, bend, who = r
    with recording() as tr:
        kw = make()
        assert key in kw or key in ("p_lp", "kl"), (name, key)
        kw[key] = bend(kw) if callable(bend) else bend
        with pytest.raises(RuntimeError) as ei:
            fn(**kw)
    return tr, ei


#: declared by the header but not called from hip_binding.py (tests and tools ask the library for its tile sizes and launch plans themselves;
#: load_library, which the stub stands in for, checks the version; the f32 head's backward is one fused call, so the
#: stand-alone fhvae_gauss_reparam_bwd has no caller)
NOT_CALLED = {"fhvae_abi_version", "fhvae_strerror", "fhvae_gauss_reparam_bwd", "fhvae_feats_tile_rows", "fhvae_kaldi_fbank_tile_rows", "fhvae_synth_tile_rows",
              "fhvae_resample_tile_rows", "fhvae_mel_invert_tile_rows", "fhvae_plan_proj", "fhvae_plan_wgrad", "fhvae_plan_gemm"}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_holds_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_match_the_pinned_trace(name, golden):
    got = json.loads(json.dumps(_run_case(name)))
    want = golden["traces"][golden["cases"][name]]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: call %d differs" % (name, k)
    assert len(got) == len(want), "%s: %d calls, pinned %d" % (name, len(got), len(want))


def test_every_symbol_the_binding_calls_is_traced(golden):
    called = {c[0] for calls in golden["traces"] for c in calls if c[0].startswith("fhvae_")}
    assert called <= set(hb.SIGNATURES)
    assert set(hb.SIGNATURES) - called == NOT_CALLED, sorted((set(hb.SIGNATURES) - called) ^ NOT_CALLED)


@pytest.mark.parametrize("r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_call(r):
    tr, ei = _run_refusal(r)
    assert r[5].split(":")[0] in str(ei.value), str(ei.value)
    assert not tr.calls


def test_shared_refusals():
    """The checks every wrapper shares: a CPU tensor (the real _need_gpu), a non-f32 operand, a schedule that changed between
    a net's forward and its backward."""
    with recording() as tr:
        hb._need_gpu = _REAL_NEED_GPU
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            hb.linear(f(3, 4), f(5, 4), f(5))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            hb.feats_fwd(**g_feats())
        assert not tr.calls
    with recording() as tr:
        with pytest.raises(RuntimeError, match="float32"):
            hb.linear(f64(3, 4), f(5, 4), f(5))
        assert not tr.calls
    ids = iter((3, 4))
    with recording(dict(fhvae_lstm_layout_id=lambda tr: next(ids))) as tr:
        x, xc, T, params, dtype, hd = _lstm_args(tr, "x", hb.F32, False, L=1)
        out, hn = hb.lstm_seq(x, xc, T, params, dtype, 2, hd)
        with pytest.raises(RuntimeError, match="schedule changed"):
            bw(tr, [out, hn])
        assert [c[0] for c in tr.calls].count("fhvae_lstm_seq_bwd") == 0


_REAL_NEED_GPU = hb._need_gpu


if __name__ == "__main__" and "--write" in sys.argv:
    traces, cases = [], {}
    for n in sorted(CASES):
        t = json.loads(json.dumps(_run_case(n)))
        if t not in traces:
            traces.append(t)
        cases[n] = traces.index(t)
    with open(GOLDEN, "w") as fh:
        fh.write('{"cases": %s,\n"traces": [\n%s\n]}\n' % (json.dumps(cases, indent=0), ",\n".join(json.dumps(t, separators=(",", ":")) for t in traces)))
    print("wrote %s (%d cases, %d traces)" % (GOLDEN, len(cases), len(traces)))
