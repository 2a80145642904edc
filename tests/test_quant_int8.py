"""_contrib_Quantization_int8 on the device (sd_quant_int8_fwd / _bwd / _weights_fwd, ops.quantization_int8_*)
against tests/quant_int8_ref.py, the float32 restatement of quantization_int8-inl.h:144-220,260-290.

Every GPU comparison is BIT-exact (out, minmax, state, dgrad): the abs-max is an unsigned maximum of bit patterns
and so order-free, and the element-wise arithmetic is fully specified (an IEEE divide, roundf, an IEEE product).
A NaN in data during a training reduction is outside the contract and is not tested."""
import ctypes

import numpy as np
import pytest

from simpledet_amd import _lib

from . import quant_int8_ref as qr

F = np.float32
P256 = ctypes.c_void_p(256)     # never dereferenced: every case that gets one fails validation first
TILE = 8192                     # elements of one workgroup trip of the abs-max pass (512 lanes x 4 x 16 bytes)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def same_bits(got, want):
    """equal bit patterns; a NaN matches a NaN (which NaN a 0 / 0 yields is the processor's choice, not the operator's)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape
    both_nan = (np.isnan(got) & np.isnan(want)).ravel()
    bad = np.flatnonzero((bits(got).ravel() != bits(want).ravel()) & ~both_nan)
    assert bad.size == 0, "first differing element %d: %r != %r (%d differ)" % (
        bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]], bad.size)


# ------------------------------------------------------------------------------------------- CPU ----
def _fwd(data=P256, out=P256, minmax=P256, state=P256, n=8, is_weight=1, is_train=1, fix=0, decay=0.99, ws=P256,
         wsb=1 << 12):
    return _lib.lib().cdll.sd_quant_int8_fwd(data, out, minmax, state, ctypes.c_long(n), is_weight, is_train, fix,
                                             ctypes.c_double(decay), ws, ctypes.c_size_t(wsb), None)


def _bwd(ograd=P256, data=P256, minmax=P256, dgrad=P256, n=8, clip=1, req=1):
    return _lib.lib().cdll.sd_quant_int8_bwd(ograd, data, minmax, dgrad, ctypes.c_long(n), clip, req, None)


def _wfwd(d=P256, o=P256, m=P256, s=P256, c=P256, T=2, n_total=8, ws=P256, wsb=1 << 20):
    return _lib.lib().cdll.sd_quant_int8_weights_fwd(d, o, m, s, c, T, ctypes.c_long(n_total), 1, 0, ws,
                                                     ctypes.c_size_t(wsb), None)


def _err():
    return (_lib.lib().cdll.sd_last_error() or b"").decode()


def test_abi_version_matches_the_header():
    assert _lib.lib().cdll.sd_abi_version() == _lib.header_abi_version()
    for name in ("sd_quant_int8_workspace_bytes", "sd_quant_int8_fwd", "sd_quant_int8_bwd",
                 "sd_quant_int8_weights_workspace_bytes", "sd_quant_int8_weights_fwd"):
        assert name in _lib.lib().protos


def test_forward_rejects_bad_arguments_before_any_launch():
    for kw in (dict(data=None), dict(out=None), dict(minmax=None), dict(state=None)):
        assert _fwd(**kw) == -1 and "null" in _err()
    assert _fwd(n=-1) == -1 and "negative" in _err()
    for decay in (-0.01, 1.01, float("nan")):
        assert _fwd(decay=decay) == -1 and "ema_decay" in _err()
    assert _fwd(data=ctypes.c_void_p(258)) == -1 and "aligned" in _err()
    assert _fwd(ws=None) == -4 and "workspace too small" in _err()
    assert _fwd(wsb=16) == -4 and "workspace too small" in _err()


def test_backward_rejects_bad_arguments_before_any_launch():
    assert _bwd(ograd=None) == -1 and "null" in _err()
    assert _bwd(dgrad=None) == -1 and "null" in _err()
    assert _bwd(data=None) == -1 and "clip" in _err()
    assert _bwd(minmax=None) == -1 and "clip" in _err()
    assert _bwd(n=-3) == -1 and "negative" in _err()
    for req in (2, 4, -1):
        assert _bwd(req=req) == -1 and "unknown req" in _err()


def test_weights_entry_point_rejects_bad_arguments_before_any_launch():
    for kw in (dict(d=None), dict(o=None), dict(m=None), dict(s=None), dict(c=None)):
        assert _wfwd(**kw) == -1 and "null" in _err()
    assert _wfwd(T=-1) == -1 and _wfwd(n_total=-1) == -1
    assert _wfwd(T=1025) == -2 and "1024" in _err()
    assert _wfwd(ws=None) == -4 and _wfwd(wsb=8) == -4 and "workspace too small" in _err()


def test_empty_problems_return_without_touching_the_device():
    # the pointers are never dereferenced and there is no GPU here: a launch would fail
    assert _fwd(n=0, ws=None, wsb=0) == 0
    assert _bwd(n=0) == 0
    assert _bwd(req=0, n=1 << 20) == 0          # req null launches nothing
    assert _wfwd(T=0, ws=None, wsb=0) == 0 and _wfwd(n_total=0, ws=None, wsb=0) == 0


def test_workspace_sizes():
    l = _lib.lib().cdll
    one = [int(l.sd_quant_int8_workspace_bytes(ctypes.c_long(n))) for n in (0, 1, 4096, 1 << 20, 1 << 33)]
    assert len(set(one)) == 1 and 0 < one[0] <= 4096          # a (max, ticket) pair and a record, whatever n is
    many = [int(l.sd_quant_int8_weights_workspace_bytes(T, ctypes.c_long(1 << 20))) for T in (1, 2, 53, 1024)]
    assert many == sorted(many) and many[0] >= one[0] - 256 and many[-1] >= 1024 * 80


def test_restatement_known_answers():
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5], dtype=F)
    # t = 127 gives u = 1: halves round away from zero
    same_bits(qr.fake_quant(x, 127.0, is_weight=False), [1, -1, 2, -2, 3, -3])
    same_bits(qr.roundf(x), [1, -1, 2, -2, 3, -3])
    edge = np.array([127, -127, 200, -200], dtype=F)
    same_bits(qr.fake_quant(edge, 127.0, is_weight=False), [127, -127, 127, -127])
    w = qr.QuantInt8Ref(is_weight=True, fix_act_scale=True, minmax=127.0)
    same_bits(w.forward(np.array([200, -200], dtype=F)), [200, -200])      # weights are not clipped
    assert w.minmax == F(127)
    with np.errstate(all="ignore"):
        assert np.isnan(qr.fake_quant(np.array([0.0, -0.0, 1.0, -3.0], dtype=F), 0.0, is_weight=False)).all()
        assert np.isnan(qr.fake_quant(np.array([0.0, 2.0], dtype=F), 0.0, is_weight=True)).all()
    # the init step: an aux below 1e-6 is replaced by the maximum, one above it is kept
    for aux, want in ((5e-7, 3.0), (2e-6, 2e-6)):
        a = qr.QuantInt8Ref(is_weight=False, minmax=aux)
        a.forward(np.array([1.0, -3.0], dtype=F))
        assert a.minmax == F(want) and a.state == [0, 0]
    # then the EMA: two rounded products and a rounded sum
    a = qr.QuantInt8Ref(is_weight=False, ema_decay=0.9, minmax=2.0)
    a.forward(np.array([1.0], dtype=F))
    a.forward(np.array([4.0], dtype=F))
    assert a.minmax == F(F(F(0.9) * F(2.0)) + F(F(F(1) - F(0.9)) * F(4.0)))
    # a delay step copies and counts down; eval quantises during the delay and changes nothing
    a = qr.QuantInt8Ref(is_weight=False, delay_quant=1, minmax=127.0)
    same_bits(a.forward(np.array([0.5], dtype=F), is_train=False), [1.0])
    assert a.state == [1, 1]
    same_bits(a.forward(np.array([0.5], dtype=F)), [0.5])
    assert a.state == [0, 1]
    # clip backward: the bounds are kept, a NaN gives 0
    a = qr.QuantInt8Ref(is_weight=False, grad_mode="clip", minmax=2.0)
    same_bits(a.backward(np.ones(5, dtype=F), np.array([2, -2, 2.0000002, -3, np.nan], dtype=F)), [1, 1, 0, 0, 0])


# ------------------------------------------------------------------------------------------- GPU ----
SIZES = (1, 3, 63, 64, 65, 255, 1027, 2 * TILE + 1, 2 ** 20 + 3)


def _data(n, seed, peak_at=None, peak=-9.5):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal(n).astype(F)
    if peak_at is not None:
        x[peak_at] = peak
    return x


def _dev(a, offset=False, dtype=None):
    """a on the device; offset: in a buffer that starts 4 bytes past a 16-byte boundary, with sentinels around"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    buf = torch.full((t.numel() + 9,), -777.0, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    v = buf[5:5 + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4
    v.sd_buf = buf
    return v


def _sentinels_intact(v):
    b = v.sd_buf.cpu().numpy()
    assert (b[:5] == -777.0).all() and (b[-4:] == -777.0).all()


class Dev:
    """the device twin of qr.QuantInt8Ref: minmax and state tensors and the operator's flags"""

    def __init__(self, ops, ref):
        import torch
        self.ops, self.ref = ops, ref
        self.minmax = torch.tensor([float(ref.minmax)], device="cuda", dtype=torch.float32)
        self.state = ops.quant_int8_state(ref.countdown, "cuda")

    def forward(self, x, is_train=True, **kw):
        r = self.ref
        return self.ops.quantization_int8_forward(x, self.minmax, self.state, is_weight=r.is_weight,
                                                  is_train=is_train, fix_act_scale=r.fix_act_scale,
                                                  ema_decay=float(r.ema_decay), **kw)

    def check_state(self):
        same_bits(self.minmax.cpu().numpy(), [self.ref.minmax])
        assert self.state.cpu().tolist() == self.ref.state


@pytest.mark.gpu
@pytest.mark.parametrize("is_weight", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_hip_sizes_and_peak_positions(ops, n, is_weight):
    for k, at in enumerate(sorted({0, n - 1, n // 2})):
        for peak in (-9.5, 7.25):
            x = _data(n, 100 + k, at, peak)
            ref = qr.QuantInt8Ref(is_weight=is_weight)
            dev = Dev(ops, ref)
            for _ in range(2):                      # activations: the init step, then an EMA step
                want = ref.forward(x)
                same_bits(dev.forward(_dev(x)).cpu().numpy(), want)
                dev.check_state()
                x = (x * F(0.5)).astype(F)
            assert ref.minmax != 0


@pytest.mark.gpu
@pytest.mark.parametrize("is_weight", [True, False])
def test_hip_exact_edge_values(ops, is_weight):
    t = F(3.1)
    u = F(t / F(127))
    ks = np.arange(-127, 127, dtype=F)
    halves = ((ks + F(0.5)) * u).astype(F)                      # quotients at or next to k + 0.5
    x = np.concatenate([[t, -t, np.nextafter(t, F(9)), -np.nextafter(t, F(9)), np.nextafter(t, F(0)),
                         -np.nextafter(t, F(0)), -0.0, 0.0, 2 * t, -2 * t, np.nan, np.inf, -np.inf],
                        halves, np.nextafter(halves, F(9)), np.nextafter(halves, F(-9))]).astype(F)
    ref = qr.QuantInt8Ref(is_weight=is_weight, fix_act_scale=True, minmax=t)
    dev = Dev(ops, ref)
    same_bits(dev.forward(_dev(x)).cpu().numpy(), ref.forward(x))
    dev.check_state()
    # u = 1: the halves themselves
    x1 = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -126.5, 127, -127, 200, -200, -0.0], dtype=F)
    ref = qr.QuantInt8Ref(is_weight=is_weight, fix_act_scale=True, minmax=127.0)
    dev = Dev(ops, ref)
    got = dev.forward(_dev(x1)).cpu().numpy()
    same_bits(got, ref.forward(x1))
    same_bits(got[:6], [1, -1, 2, -2, 3, -3])
    same_bits(got[-3:], [200, -200, -0.0] if is_weight else [127, -127, -0.0])
    # t = 0: NaN everywhere, as the reference's arithmetic gives
    ref = qr.QuantInt8Ref(is_weight=is_weight)
    dev = Dev(ops, ref)
    z = np.zeros(70, dtype=F)
    got = dev.forward(_dev(z)).cpu().numpy()
    assert np.isnan(got).all() and np.isnan(ref.forward(z)).all()
    dev.check_state()


def _sequence(ops, n=1027, graph=False, **ref_kw):
    """five training steps on five inputs, then an eval call; state and minmax checked after each"""
    import torch
    ref = qr.QuantInt8Ref(**ref_kw)
    dev = Dev(ops, ref)
    xs = [(_data(n, 7 + i, (i * 211) % n, (-1) ** i * (3.0 + i))) for i in range(5)]
    if graph:
        x_d = _dev(xs[0])
        out_d = torch.empty_like(x_d)
        ws = torch.empty(ops.quant_int8_workspace_bytes(n), device="cuda", dtype=torch.uint8)
        keep = (dev.minmax.clone(), dev.state.clone())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dev.forward(x_d, out=out_d, workspace=ws)            # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        dev.minmax.copy_(keep[0])
        dev.state.copy_(keep[1])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            dev.forward(x_d, out=out_d, workspace=ws)
        dev.minmax.copy_(keep[0])                                 # a capture runs nothing; be explicit anyway
        dev.state.copy_(keep[1])
    modes = []
    for x in xs:
        before = ref.state
        want = ref.forward(x)
        if graph:
            x_d.copy_(torch.from_numpy(x))
            g.replay()
            got = out_d.cpu().numpy()
        else:
            got = dev.forward(_dev(x)).cpu().numpy()
        same_bits(got, want)
        dev.check_state()
        modes.append("copy" if before[0] > 0 else ("init" if before[1] else "ema"))
    if not graph:
        mm, st = bits(dev.minmax.cpu().numpy()).copy(), dev.state.cpu().tolist()
        x = _data(n, 99, 5, 40.0)
        same_bits(dev.forward(_dev(x), is_train=False).cpu().numpy(), ref.forward(x, is_train=False))
        assert (bits(dev.minmax.cpu().numpy()) == mm).all() and dev.state.cpu().tolist() == st
    return modes, ref


@pytest.mark.gpu
def test_hip_five_step_activation_sequence_and_eval(ops):
    modes, ref = _sequence(ops, is_weight=False, delay_quant=2)
    assert modes == ["copy", "copy", "init", "ema", "ema"] and ref.state == [0, 0]
    # the eval call during the delay quantises and leaves the state alone
    ref = qr.QuantInt8Ref(is_weight=False, delay_quant=2, minmax=1.5)
    dev = Dev(ops, ref)
    x = _data(300, 3)
    same_bits(dev.forward(_dev(x), is_train=False).cpu().numpy(), ref.forward(x, is_train=False))
    dev.check_state()
    assert ref.state == [2, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(is_weight=True), dict(is_weight=True, fix_act_scale=True, minmax=1.5),
                                dict(is_weight=False, fix_act_scale=True, minmax=1.5),
                                dict(is_weight=False, minmax=1.5), dict(is_weight=False, ema_decay=0.9),
                                dict(is_weight=False, ema_decay=0.0), dict(is_weight=False, ema_decay=1.0),
                                dict(is_weight=False, ema_decay=0.99, n=2 * TILE + 1)],
                         ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_hip_sequences(ops, kw):
    kw = dict(kw)
    modes, ref = _sequence(ops, delay_quant=2, **kw)
    assert modes[:2] == ["copy", "copy"]
    if kw.get("fix_act_scale"):
        assert ref.minmax == F(1.5)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1027, 3 * TILE + 5])
def test_hip_graph_replay_equals_the_eager_sequence(ops, n):
    modes, ref = _sequence(ops, n=n, graph=True, is_weight=False, delay_quant=2)
    assert modes == ["copy", "copy", "init", "ema", "ema"] and ref.state == [0, 0]
    # the eager run of the same five inputs is held to the same restatement, step by step
    _sequence(ops, n=n, is_weight=False, delay_quant=2)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 1027, 2 * TILE + 1])
def test_hip_offset_pointers_give_the_same_bits_and_stay_in_bounds(ops, n):
    import torch
    x = _data(n, 21, n - 1, -6.0)
    g = _data(n, 22)
    for off_in, off_out in ((True, True), (True, False), (False, True)):
        for is_weight in (True, False):
            ref = qr.QuantInt8Ref(is_weight=is_weight, grad_mode="clip")
            dev = Dev(ops, ref)
            out = _dev(np.zeros(n, dtype=F), off_out)
            dev.forward(_dev(x, off_in), out=out)
            same_bits(out.cpu().numpy(), ref.forward(x))
            dev.check_state()
            if off_out:
                _sentinels_intact(out)
            x2 = (x * F(1.7)).astype(F)      # some elements beyond the threshold now
            d = _dev(np.full(n, 0.25, dtype=F), off_out)
            ops.quantization_int8_backward(_dev(g, off_in), _dev(x2, not off_in), dev.minmax, is_weight=is_weight,
                                           grad_mode="clip", req="add", d_data=d)
            same_bits(d.cpu().numpy(), F(0.25) + ref.backward(g, x2))
            if off_out:
                _sentinels_intact(d)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [7, 1027, 2 * TILE + 1])
def test_hip_backward_modes(ops, n):
    import torch
    t = F(1.25)
    x = _data(n, 31)
    x[:6] = [t, -t, np.nextafter(t, F(9)), -np.nextafter(t, F(9)), np.nan, -0.0]
    g = _data(n, 32)
    mm = torch.tensor([float(t)], device="cuda")
    for is_weight, mode in ((False, "ste"), (True, "ste"), (True, "clip"), (False, "clip")):
        ref = qr.QuantInt8Ref(is_weight=is_weight, grad_mode=mode, minmax=t)
        want = ref.backward(g, x)
        got = ops.quantization_int8_backward(_dev(g), _dev(x), mm, is_weight=is_weight, grad_mode=mode)
        same_bits(got.cpu().numpy(), want)
        if mode == "clip" and not is_weight:
            same_bits(want[:5], [g[0], g[1], 0, 0, 0])      # the bounds are kept, a NaN gives +0.0
        acc = _dev(np.arange(n, dtype=F) + F(1))
        ops.quantization_int8_backward(_dev(g), _dev(x), mm, is_weight=is_weight, grad_mode=mode, req="add",
                                       d_data=acc)
        same_bits(acc.cpu().numpy(), (np.arange(n, dtype=F) + F(1)) + want)
        kept = _dev(np.full(n, 5.0, dtype=F))
        ops.quantization_int8_backward(_dev(g), _dev(x), mm, is_weight=is_weight, grad_mode=mode, req="null",
                                       d_data=kept)
        assert (kept.cpu().numpy() == 5.0).all()


MULTI_SIZES = (1, 5, 64, 1027, 4096, 36864, 2 ** 18 + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("is_train,fix", [(True, False), (True, True), (False, False)])
def test_hip_multi_tensor_equals_single_calls_and_the_restatement(ops, is_train, fix):
    import torch
    xs = [_data(n, 50 + i, (n * 3) // 4, (-1) ** i * (2.0 + i)) for i, n in enumerate(MULTI_SIZES)]
    delays = [0, 0, 0, 1, 0, 0, 0]                                   # the fourth is still in its delay
    auxs = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    refs = [qr.QuantInt8Ref(is_weight=True, delay_quant=d, fix_act_scale=fix, minmax=a) for d, a in zip(delays, auxs)]
    multi = [Dev(ops, r) for r in refs]
    single = [Dev(ops, r) for r in refs]
    datas = [_dev(x, offset=(i % 2 == 1)) for i, x in enumerate(xs)]
    outs = [_dev(np.zeros_like(x), offset=(i % 3 == 1)) for i, x in enumerate(xs)]
    table = ops.quant_int8_weights_table(datas, outs, [m.minmax for m in multi], [m.state for m in multi])
    for step in range(2):
        got = ops.quantization_int8_weights_forward(datas, [m.minmax for m in multi], [m.state for m in multi],
                                                    is_train=is_train, fix_act_scale=fix, outs=outs, table=table)
        for i, x in enumerate(xs):
            one = single[i].forward(_dev(x), is_train=is_train)
            want = refs[i].forward(x, is_train=is_train)
            same_bits(got[i].cpu().numpy(), want)
            same_bits(one.cpu().numpy(), want)
            multi[i].check_state()
            single[i].check_state()
            if i % 3 == 1:
                _sentinels_intact(outs[i])
    torch.cuda.synchronize()
    if is_train:
        assert refs[3].state == [0, 1]


@pytest.mark.gpu
def test_hip_autograd_round_trip(ops):
    import torch
    x = _data(1027, 61, 9, -4.0)
    g = _data(1027, 62)
    for is_weight, mode in ((True, "ste"), (False, "clip")):
        ref = qr.QuantInt8Ref(is_weight=is_weight, grad_mode=mode)
        dev = Dev(ops, ref)
        xd = _dev(x).reshape(13, 79).requires_grad_(True)
        y = ops.quantization_int8(xd, dev.minmax, dev.state, is_weight=is_weight, grad_mode=mode)
        same_bits(y.detach().cpu().numpy().ravel(), ref.forward(x))
        dev.check_state()
        y.backward(_dev(g).reshape(13, 79))
        same_bits(xd.grad.cpu().numpy().ravel(), ref.backward(g, x))
    with pytest.raises(ValueError):
        ops.quantization_int8(_dev(x), dev.minmax, dev.state, grad_mode="other")
    with pytest.raises(ValueError):
        ops.quantization_int8_forward(_dev(x), dev.minmax, dev.state, is_weight=True, ema_decay=1.5)


# Above 512 units of one trip the abs-max pass gives a workgroup several trips (n > 512 * 8192), above 2048 units
# the element-wise pass and the backward do (n > 2048 * 4096): every activation of the int8 config is there.
BIG = 2 * 64 * 200 * 336 + 3        # the (2, 64, 200, 336) activation and a tail: 8 601 603 elements
assert BIG > 2048 * 4096


@pytest.fixture(scope="module")
def big():
    x = _data(BIG, 71, BIG - 2, -5.5)
    x[:4] = [5.5, -5.5, 5.4999995, np.nan]      # the NaN is seen only by calls that do not reduce
    return x, _data(BIG, 72)


@pytest.mark.gpu
def test_hip_several_trips_per_workgroup_forward_eval_backward(ops, big):
    x, g = big
    xt = x.copy()
    xt[3] = 0.25                                  # a training reduction never sees a NaN
    for is_weight in (False, True):
        ref = qr.QuantInt8Ref(is_weight=is_weight, grad_mode="clip", minmax=2.0)
        ref.init = 0                              # past the init step: an EMA step for the activation
        dev = Dev(ops, ref)
        dev.state[1] = 0
        out = _dev(np.zeros(BIG, dtype=F), True)
        dev.forward(_dev(xt, True), out=out)
        same_bits(out.cpu().numpy(), ref.forward(xt))
        dev.check_state()
        _sentinels_intact(out)
        out = _dev(np.zeros(BIG, dtype=F), True)
        dev.forward(_dev(x), out=out, is_train=False)        # eval: the element-wise pass alone
        same_bits(out.cpu().numpy(), ref.forward(x, is_train=False))
        dev.check_state()
        _sentinels_intact(out)
    d = _dev(np.full(BIG, 0.25, dtype=F), True)
    ops.quantization_int8_backward(_dev(g, True), _dev(x), dev.minmax, is_weight=False, grad_mode="clip", req="add",
                                   d_data=d)
    ref = qr.QuantInt8Ref(is_weight=False, grad_mode="clip", minmax=dev.ref.minmax)
    same_bits(d.cpu().numpy(), F(0.25) + ref.backward(g, x))
    _sentinels_intact(d)


@pytest.mark.gpu
def test_hip_multi_tensor_with_units_of_several_trips(ops, big):
    x = big[0].copy()
    x[3] = 0.25
    cuts = [0, 1, 8192 * 3 + 1, 8192 * 3 + 1 + 1027, BIG - 70001, BIG]       # five tensors, one of 8.5 M elements
    xs = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    refs = [qr.QuantInt8Ref(is_weight=True, delay_quant=int(i == 2), minmax=0.5 * i) for i in range(len(xs))]
    devs = [Dev(ops, r) for r in refs]
    datas = [_dev(v, offset=(i % 2 == 1)) for i, v in enumerate(xs)]
    outs = [_dev(np.zeros_like(v), offset=True) for v in xs]
    for step in range(2):
        got = ops.quantization_int8_weights_forward(datas, [m.minmax for m in devs], [m.state for m in devs],
                                                    outs=outs)
        for i, v in enumerate(xs):
            same_bits(got[i].cpu().numpy(), refs[i].forward(v))
            devs[i].check_state()
            _sentinels_intact(outs[i])
    assert refs[2].state == [0, 1]
