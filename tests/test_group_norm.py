"""_contrib_GroupNorm (simpledet_amd/csrc/group_norm.hip) against the restatements of tests/group_norm_ref.py.

  CPU: argument validation of the three C entry points (every case fails, or succeeds, before any launch);
       the workspace size is monotone in N and C; the float32 restatement of the reference stays finite over
       the sweep (its k per output is printed).
  GPU: within a margin, per case and per output (y, mu, rsig, dx, dgamma, dbeta):
           k = |got - truth| / (eps32 * T + tiny)                                (tests/group_norm_ref.py)
           k_gpu <= 2 * k_ref(case) + 2,
       k_ref = the float32 restatement's own k on the same case, computed in the same run: a factor 2 for the
       free reduction order plus 2 units for the final roundings, the margin rule of tests/test_focal_loss.py;
       on the zero-offset cases additionally k_gpu <= 2 * (max over the zero-offset cases of k_ref) + 2, so that
       the loose bound of a high-offset case (where the reference's E[x^2] - mu^2 cancels) hides nothing.
       Exactly: a constant group, gamma == 0 channels, dbeta of an all-ones dY, sentinels around every output
       and behind the N*G floats of an (N, C) mean / var buffer, equal bits from two calls, from a captured
       graph and from pointers off their 16-byte boundary, the dispatch taken per regime, autograd.
       tools/group_norm_time.py stores the measured k_ref / k_gpu in profiles/group_norm_time.json under 'margin'
       (DESIGN.md 4.10).
"""
import ctypes
import functools

import numpy as np
import pytest

from simpledet_amd import _lib

from . import group_norm_ref as gr

P = ctypes.c_void_p(256)   # never dereferenced: every CPU case returns before any launch


# ------------------------------------------------------------------------------------------ CPU --
def _wsb(N, C, HxW, G):
    fn = _lib.lib().cdll.sd_group_norm_workspace_bytes
    return int(fn(N, C, ctypes.c_long(HxW), G))


def _fwd(N=2, C=8, HxW=16, G=4, ptr=P, ws=P, wsb=None, skip=()):
    a = [None if i in skip else ptr for i in range(6)]
    wsb = _wsb(N, C, HxW, G) if wsb is None else wsb
    return _lib.lib().call("sd_group_norm_fwd", *a, N, C, ctypes.c_long(HxW), G, ctypes.c_float(1e-5), ws,
                           ctypes.c_size_t(wsb), None)


def _bwd(N=2, C=8, HxW=16, G=4, ptr=P, ws=P, wsb=None, skip=(), dgamma=P, dbeta=P):
    a = [None if i in skip else ptr for i in range(6)]
    wsb = _wsb(N, C, HxW, G) if wsb is None else wsb
    return _lib.lib().call("sd_group_norm_bwd", *a, dgamma, dbeta, N, C, ctypes.c_long(HxW), G, ws,
                           ctypes.c_size_t(wsb), None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_entry_points_reject_bad_arguments_without_a_gpu(call):
    E = _lib.SimpleDetOpsError
    for kw in (dict(N=-1), dict(C=-8), dict(HxW=-1)):
        with pytest.raises(E, match="negative dimension") as e:
            call(**kw)
        assert e.value.code == -1
    for G in (0, -4):
        with pytest.raises(E, match="not positive") as e:
            call(G=G)
        assert e.value.code == -1
    with pytest.raises(E, match="not divisible") as e:
        call(C=10, G=4)
    assert e.value.code == -1
    for i in range(6):
        with pytest.raises(E, match="null pointer") as e:
            call(skip=(i,))
        assert e.value.code == -1
    with pytest.raises(E, match="workspace too small") as e:
        call(wsb=_wsb(2, 8, 16, 4) - 1)
    assert e.value.code == -1
    with pytest.raises(E, match="workspace too small"):
        call(ws=None)
    # 2^31 - 1 elements is the stated limit: 2 x 1024 x 1048576 = 2^31
    with pytest.raises(E, match="exceed the limit") as e:
        call(N=2, C=1024, HxW=1 << 20, G=32, wsb=1 << 30)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(E, match="exceed the limit"):
        call(N=1 << 20, C=1 << 20, HxW=1 << 40, G=1, wsb=1 << 30)
    # empty problems succeed without touching the device (no pointer, no workspace)
    assert call(N=0, ptr=None, ws=None, wsb=0) == 0
    assert call(HxW=0, ptr=None, ws=None, wsb=0) == 0
    # ... but their parameters are still checked
    with pytest.raises(E, match="not divisible"):
        call(N=0, C=10, G=4, ptr=None, ws=None, wsb=0)


def test_backward_takes_dgamma_and_dbeta_together_or_not_at_all():
    with pytest.raises(_lib.SimpleDetOpsError, match="together") as e:
        _bwd(dgamma=None)
    assert e.value.code == -1
    with pytest.raises(_lib.SimpleDetOpsError, match="together"):
        _bwd(dbeta=None)
    assert _bwd(N=0, dgamma=None, dbeta=None, ptr=None, ws=None, wsb=0) == 0


def test_workspace_bytes_is_monotone_in_n_and_c():
    for HxW, G in ((49, 32), (196, 32), (67200, 32), (1050, 1)):
        prev = 0
        for N in (1, 2, 3, 8, 64, 1024):
            if N * 256 * HxW >= 1 << 31:      # (beyond the limit of the entry points the size is not defined)
                continue
            b = _wsb(N, 256, HxW, G)
            assert b >= prev
            prev = b
        prev = 0
        for C in (G, 2 * G, 8 * G, 64 * G):
            b = _wsb(2, C, HxW, G)
            assert b >= prev
            prev = b
    assert _wsb(2, 256, 67200, 32) >= 2 * 256 * 2 * 4          # the (N, C, 2) table of the backward
    assert 0 < _wsb(0, 256, 49, 32) <= 4096 and 0 < _wsb(2, 256, 49, 0) <= 4096


@functools.lru_cache(maxsize=None)
def _cases():
    return gr.cases()


@functools.lru_cache(maxsize=None)
def _evaluated():
    return [(name, c) + gr.evaluate(c) for name, c in _cases()]


def test_restatements_agree():
    """The float32 restatement of the reference against the float64 truth over the sweep: finite on every case
    (at offsets of 0, 3 and 100 standard deviations the relative error of E[x^2] - mu^2 is about eps32 * 10^4
    at most, far from a negative variance).  The figures are printed; no bound on them is asserted, they are the
    yardstick the device is held to."""
    worst = {o: (0.0, None) for o in gr.OUTPUTS}
    by_off = {}
    for name, c, truth, T, k_ref, _, _ in _evaluated():
        for o in gr.OUTPUTS:
            assert np.isfinite(k_ref[o]), (name, o, k_ref[o])
            if k_ref[o] > worst[o][0]:
                worst[o] = (k_ref[o], name)
            key = (c["offset"], o)
            by_off[key] = max(by_off.get(key, 0.0), k_ref[o])
    for o in gr.OUTPUTS:
        print("k_ref %-6s max %.3f (%s)   by offset: %s" % (
            o, worst[o][0], worst[o][1], "  ".join("%g: %.3f" % (off, by_off[(off, o)]) for off in gr.OFFSETS)))
    # the constant group: variance exactly 0 and rsig = 1 / sqrt(eps) exactly, in the restatement and the truth
    name, c, truth, T, k_ref, mu32, rs32 = _evaluated()[-1]
    assert name == "constant"
    f32 = gr.fwd_f32(c["x"], c["gamma"], c["beta"], c["G"], c["eps"])
    want = np.float32(1.0) / np.sqrt(np.float32(0.0) + np.float32(c["eps"]))
    assert f32["mu"][0, 1] == 1.5 and f32["rsig"][0, 1] == want and rs32[0, 1] == want and mu32[0, 1] == 1.5


def test_restatement_known_answer():
    """x = [1, 3] per group, gamma = 2, beta = 1, eps = 0: mu = 2, var = 1, y = [-1, 3]; dy = [1, 0]:
    ds = 2 * 1, db = 2, dx = 2 * dy + ((2 * 2 - 2) * (x - 2) - 2) / 2 = [2 + (-2 - 2) / 2, (2 - 2) / 2] = [0, 0]
    (the gradient of a two-point normalisation vanishes), dgamma = dy * (x - mu) = -1, dbeta = 1."""
    x = np.float32([[[1.0, 3.0]]]).reshape(1, 1, 2)
    g, b, dy = np.float32([2.0]), np.float32([1.0]), np.float32([1.0, 0.0]).reshape(1, 1, 2)
    for f in (gr.fwd_f32, lambda *a: gr.fwd_truth(*a)[0]):
        r = f(x, g, b, 1, 0.0)
        assert r["mu"].item() == 2.0 and r["rsig"].item() == 1.0 and r["y"].reshape(-1).tolist() == [-1.0, 3.0]
    for f in (gr.bwd_f32, lambda *a: gr.bwd_truth(*a)[0]):
        r = f(dy, x, np.float32([[2.0]]), np.float32([[1.0]]), g, 1)
        assert r["dx"].reshape(-1).tolist() == [0.0, 0.0] and r["dgamma"].item() == -1.0 and r["dbeta"].item() == 1.0
    T = gr.bwd_truth(dy, x, np.float32([[2.0]]), np.float32([[1.0]]), g, 1)[1]
    # Tds = 2, Tdb = 2: first element 2 + ((2 * 2 + 2) * (1 + 2) + 2) / 2 = 12
    assert T["dx"].reshape(-1)[0] == 12.0 and T["dgamma"].item() == 3.0 and T["dbeta"].item() == 1.0


# ------------------------------------------------------------------------------------------ GPU --
def _cuda(a, offset=False, fill=None):
    """a device copy; offset: the data pointer sits 4 bytes off its 16-byte boundary (scalar path)"""
    import torch
    a = np.ascontiguousarray(a, np.float32)
    if not offset:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4
    return t


def _run(ops, c, mu32, rs32, offset=False):
    """forward, then the backward on the float32 roundings of the true mu / rsig -> dict of numpy outputs"""
    import torch
    x, dy, g, b = _cuda(c["x"], offset), _cuda(c["dy"], offset), _cuda(c["gamma"]), _cuda(c["beta"])
    nan = np.full(c["x"].shape, np.nan, np.float32)
    y, mu, rsig = ops.group_norm_forward(x, g, b, c["G"], c["eps"], y=_cuda(nan, offset))
    dx, dgamma, dbeta = ops.group_norm_backward(dy, x, _cuda(mu32), _cuda(rs32), g, c["G"], dx=_cuda(nan, offset))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(y=y, mu=mu, rsig=rsig, dx=dx, dgamma=dgamma, dbeta=dbeta).items()}


@pytest.mark.gpu
def test_hip_group_norm_margin(ops):
    ev = _evaluated()
    zero_ref = {o: max(k_ref[o] for _, c, _, _, k_ref, _, _ in ev if c["offset"] == 0.0) for o in gr.OUTPUTS}
    worst = {o: (0.0, 0.0, None) for o in gr.OUTPUTS}
    worst0 = {o: 0.0 for o in gr.OUTPUTS}
    failures = []
    for i, (name, c, truth, T, k_ref, mu32, rs32) in enumerate(ev):
        got = _run(ops, c, mu32, rs32, offset=i % 5 == 3)      # every fifth case off the 16-byte boundary
        for o in gr.OUTPUTS:
            k = gr.k_of(got[o], truth[o], T[o])
            if k > worst[o][0]:
                worst[o] = (k, k_ref[o], name)
            if not k <= 2 * k_ref[o] + 2:
                failures.append("%s %s: k_gpu %.3f > 2 * %.3f + 2" % (name, o, k, k_ref[o]))
            if c["offset"] == 0.0:
                worst0[o] = max(worst0[o], k)
                if not k <= 2 * zero_ref[o] + 2:
                    failures.append("%s %s (zero offset): k_gpu %.3f > 2 * %.3f + 2" % (name, o, k, zero_ref[o]))
    for o in gr.OUTPUTS:
        print("group_norm %-6s: worst k_gpu %.3f (k_ref %.3f there, %s); zero offset: k_gpu %.3f against k_ref %.3f"
              % ((o,) + worst[o] + (worst0[o], zero_ref[o])))
    assert not failures, "\n".join(failures[:20])


@pytest.mark.gpu
def test_hip_backward_margin_on_the_device_forward_statistics(ops):
    """forward -> backward chained on the device's OWN mu / rsig (what a train step does): the truth and the
    restatement's k_ref are then formed from those same float32 arrays, the inputs the backward was given.
    The same bound: k_gpu <= 2 * k_ref + 2 per case and output.  One case per shape, offset and gamma kind."""
    import torch
    failures, worst = [], {o: (0.0, 0.0, None) for o in ("dx", "dgamma", "dbeta")}
    for name, c in [e for e in _cases() if e[0].endswith("eps1e-05") or e[0] == "constant"]:
        x, dy, g, b = _cuda(c["x"]), _cuda(c["dy"]), _cuda(c["gamma"]), _cuda(c["beta"])
        y, mu, rsig = ops.group_norm_forward(x, g, b, c["G"], c["eps"])
        dx, dgamma, dbeta = ops.group_norm_backward(dy, x, mu, rsig, g, c["G"])
        torch.cuda.synchronize()
        mu_d, rs_d = mu.cpu().numpy(), rsig.cpu().numpy()
        truth, T = gr.bwd_truth(c["dy"], c["x"], mu_d, rs_d, c["gamma"], c["G"])
        ref = gr.bwd_f32(c["dy"], c["x"], mu_d, rs_d, c["gamma"], c["G"])
        for o, got in (("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
            k, k_ref = gr.k_of(got.cpu().numpy(), truth[o], T[o]), gr.k_of(ref[o], truth[o], T[o])
            if k > worst[o][0]:
                worst[o] = (k, k_ref, name)
            if not k <= 2 * k_ref + 2:
                failures.append("%s %s: k_gpu %.3f > 2 * %.3f + 2" % (name, o, k, k_ref))
    for o, w in worst.items():
        print("group_norm chained %-6s: worst k_gpu %.3f (k_ref %.3f there, %s)" % ((o,) + w))
    assert not failures, "\n".join(failures[:20])


@pytest.mark.gpu
def test_hip_constant_group_and_zero_gamma_are_exact(ops):
    name, c, truth, T, k_ref, mu32, rs32 = _evaluated()[-1]
    got = _run(ops, c, mu32, rs32)
    beta = c["beta"]
    assert np.all(got["mu"][0, 1] == 1.5)
    assert got["rsig"][0, 1] == np.float32(1.0) / np.sqrt(np.float32(c["eps"]))
    for ch in range(4, 8):
        assert np.all(got["y"][0, ch] == beta[ch]), ch
    assert np.isfinite(got["dx"]).all() and np.isfinite(got["dgamma"]).all()
    # gamma == 0 channels: y is beta exactly, and their dy reaches no dx (not their own, not their group's)
    for name, c, truth, T, k_ref, mu32, rs32 in [e for e in _evaluated() if "-zeros-off3-eps1e-05" in e[0]]:
        zero = np.flatnonzero(c["gamma"] == 0)
        assert zero.size
        got = _run(ops, c, mu32, rs32)
        for ch in zero:
            assert np.all(got["y"][:, ch] == c["beta"][ch]), (name, ch)
        c2 = dict(c, dy=c["dy"].copy())
        c2["dy"][:, zero] *= -3.0
        got2 = _run(ops, c2, mu32, rs32)
        # (equal VALUES: where a whole group has gamma == 0 -- G = C -- dx is 0 * dy + ..., a zero whose sign is dy's;
        # in every channel with gamma != 0 the bits are equal too)
        assert np.isfinite(got["dx"]).all() and np.array_equal(got["dx"], got2["dx"]), name
        live = c["gamma"] != 0
        assert np.array_equal(got["dx"][:, live].view(np.int32), got2["dx"][:, live].view(np.int32)), name


@pytest.mark.gpu
def test_hip_dbeta_of_ones_is_the_count(ops):
    rs = np.random.RandomState(9)
    for shape, G in (((8, 64, 7, 7), 32), ((2, 64, 100, 168), 32), ((2, 16, 5, 9), 4), ((3, 32, 24, 24), 4)):
        N, C = shape[:2]
        count = N * int(np.prod(shape[2:]))
        assert count < 1 << 24
        c = gr.make_case(rs, shape, G, "random", 0.0, 1e-5)
        c["dy"] = np.ones(shape, np.float32)
        ft, _ = gr.fwd_truth(c["x"], c["gamma"], c["beta"], G, c["eps"])
        got = _run(ops, c, ft["mu"].astype(np.float32), ft["rsig"].astype(np.float32))
        assert np.all(got["dbeta"] == np.float32(count)), (shape, got["dbeta"][:4], count)


def _dispatch():
    return (_lib.lib().cdll.sd_last_dispatch() or b"").decode()


@pytest.mark.gpu
def test_hip_both_regimes_are_reached(ops):
    import torch
    seen = {}
    for shape in ((1024, 256, 7, 7), (256, 256, 14, 14), (2, 256, 200, 336)):
        x = torch.randn(shape, device="cuda")
        g, b = torch.randn(256, device="cuda"), torch.randn(256, device="cuda")
        y, mu, rsig = ops.group_norm_forward(x, g, b, 32)
        f = _dispatch()
        ops.group_norm_backward(x, x, mu, rsig, g, 32)
        seen[shape] = (f, _dispatch())
        torch.cuda.synchronize()
        del x, y
    for shape in ((1024, 256, 7, 7), (256, 256, 14, 14)):
        for d in seen[shape]:
            assert "small_kernel" in d and "split" not in d, (shape, d)
    assert "scalar" in seen[(1024, 256, 7, 7)][0] and "vec4" in seen[(256, 256, 14, 14)][0]   # 49 is odd: scalar
    for d in seen[(2, 256, 200, 336)]:
        assert "(split)" in d and "small" not in d, d
    assert "gn_fwd_partial_kernel<vec4>" in seen[(2, 256, 200, 336)][0]
    assert "gn_bwd_rows_kernel<256,vec4>" in seen[(2, 256, 200, 336)][1]


SENTINEL = -12345.5


def _carve(buf, start, shape):
    n = int(np.prod(shape))
    return buf[start:start + n].view(shape)


@pytest.mark.gpu
def test_hip_outputs_leave_their_surroundings_alone(ops):
    """every output carved from the middle of a sentinel-filled buffer (and the workspace from a sentinel-filled
    byte buffer); mean / var of the reference's declared shape (N, C) keep the sentinel behind their N*G floats"""
    import torch
    rs = np.random.RandomState(11)
    for shape, G, off in (((8, 64, 7, 7), 32, 4), ((4, 32, 14, 14), 8, 4), ((2, 64, 100, 168), 32, 8),
                          ((2, 32, 24, 24), 4, 3), ((2, 64, 7, 7), 1, 5)):
        N, C = shape[:2]
        c = gr.make_case(rs, shape, G, "random", 3.0, 1e-5)
        x, dy, g, b = _cuda(c["x"]), _cuda(c["dy"]), _cuda(c["gamma"]), _cuda(c["beta"])
        n = x.numel()
        pad = 1024 + off                                   # off: 16-byte alignment of y / dx where off % 4 == 0
        big = {k: torch.full((n + 2 * pad,), SENTINEL, device="cuda") for k in ("y", "dx")}
        small = {k: torch.full((N * C + 2 * pad,), SENTINEL, device="cuda") for k in ("mu", "rsig", "dgamma", "dbeta")}
        wsb = ops.group_norm_workspace_bytes(N, C, n // (N * C), G)
        wsbuf = torch.full((wsb + 2 * 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        ws = wsbuf[4096:4096 + wsb]
        mu, rsig = _carve(small["mu"], pad, (N, C)), _carve(small["rsig"], pad, (N, C))
        y, mu_, rsig_ = ops.group_norm_forward(x, g, b, G, c["eps"], y=_carve(big["y"], pad, shape), mu=mu, rsig=rsig,
                                               workspace=ws)
        ops.group_norm_backward(dy, x, mu, rsig, g, G, dx=_carve(big["dx"], pad, shape),
                                dgamma=_carve(small["dgamma"], pad, (C,)), dbeta=_carve(small["dbeta"], pad, (C,)),
                                workspace=ws)
        torch.cuda.synchronize()
        plain = ops.group_norm_forward(x, g, b, G, c["eps"])
        pb = ops.group_norm_backward(dy, x, plain[1], plain[2], g, G)
        for k, t in big.items():
            assert torch.all(t[:pad] == SENTINEL) and torch.all(t[pad + n:] == SENTINEL), (shape, k)
        for k, used in (("mu", N * G), ("rsig", N * G), ("dgamma", C), ("dbeta", C)):
            t = small[k]
            assert torch.all(t[:pad] == SENTINEL) and torch.all(t[pad + used:] == SENTINEL), (shape, k)
            assert not torch.any(t[pad:pad + used] == SENTINEL), (shape, k)
        assert torch.all(wsbuf[:4096] == 0xA5) and torch.all(wsbuf[4096 + wsb:] == 0xA5), shape
        if off % 4 == 0:    # (the same alignment class: the same kernels, so the same bits)
            assert torch.equal(y, plain[0]) and torch.equal(_carve(big["dx"], pad, shape), pb[0])
            assert torch.equal(mu.reshape(-1)[:N * G], plain[1].reshape(-1))
            assert torch.equal(_carve(small["dgamma"], pad, (C,)), pb[1])


@pytest.mark.gpu
def test_hip_two_calls_and_a_captured_graph_give_equal_bits(ops):
    import torch
    rs = np.random.RandomState(12)
    for shape, G in (((8, 64, 7, 7), 32), ((2, 64, 100, 168), 32), ((2, 32, 24, 24), 4)):
        N, C = shape[:2]
        c = gr.make_case(rs, shape, G, "random", 3.0, 1e-5)
        x, dy, g, b = _cuda(c["x"]), _cuda(c["dy"]), _cuda(c["gamma"]), _cuda(c["beta"])

        def both(**kw):
            y, mu, rsig = ops.group_norm_forward(x, g, b, G, c["eps"], workspace=kw.get("ws1"))
            dx, dgamma, dbeta = ops.group_norm_backward(dy, x, mu, rsig, g, G, workspace=kw.get("ws2"))
            return y, mu, rsig, dx, dgamma, dbeta
        eager = [t.clone() for t in both()]
        again = both()
        for e, a in zip(eager, again):
            assert torch.equal(e.view(torch.int32), a.view(torch.int32))
        wsb = ops.group_norm_workspace_bytes(N, C, x.numel() // (N * C), G)
        ws1 = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        ws2 = torch.empty_like(ws1)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                cap = both(ws1=ws1, ws2=ws2)
        for _ in range(2):
            for t in cap:
                t.fill_(float("nan"))
            ws1.fill_(0xFF)
            ws2.fill_(0xFF)
            graph.replay()
            torch.cuda.synchronize()
            for e, t in zip(eager, cap):
                assert torch.equal(e.view(torch.int32), t.view(torch.int32)), shape
        # kernel nodes only: nothing in the captured call is a memset or a copy
        kinds = _node_types(lambda: both(ws1=ws1, ws2=ws2))
        assert len(kinds) >= 3 and all(k == 0 for k in kinds), (shape, kinds)       # hipGraphNodeTypeKernel = 0


def _hip_runtime():
    """the HIP runtime this process already has loaded (torch's), for hipGraphGetNodes / hipGraphNodeGetType"""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return ctypes.CDLL(path)
    pytest.fail("no libamdhip64 is mapped into this process")


def _node_types(fn):
    """capture fn() into a graph that is kept (not instantiated) and list the type of every node"""
    import torch
    hip = _hip_runtime()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            keep = fn()
    raw = ctypes.c_void_p(int(graph.raw_cuda_graph()))
    n = ctypes.c_size_t(0)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0 and n.value > 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) == 0
    kinds = []
    for i in range(n.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)) == 0
        kinds.append(t.value)
    del keep
    return kinds


@pytest.mark.gpu
def test_hip_offset_pointers_leave_the_16_byte_path_and_give_the_same_bits(ops):
    """x, y, dy and dx 4 bytes off their 16-byte boundary: no 16-byte access is issued (the 'quad' kernels move
    the same four-float items by 4-byte accesses, so every sum keeps its order) and no bit of any output changes.
    An odd HxW is on the one-float path wherever its pointers lie."""
    import torch
    rs = np.random.RandomState(13)
    for shape, G, modes in (((4, 32, 14, 14), 8, ("vec4", "quad")), ((2, 64, 100, 168), 32, ("vec4", "quad")),
                            ((2, 32, 24, 24), 4, ("vec4", "quad")), ((8, 64, 7, 7), 32, ("scalar", "scalar")),
                            ((2, 64, 25, 42), 2, ("scalar", "scalar"))):
        c = gr.make_case(rs, shape, G, "random", 3.0, 1e-5)
        g, b = _cuda(c["gamma"]), _cuda(c["beta"])
        res = []
        for offset, mode in zip((False, True), modes):
            x, dy = _cuda(c["x"], offset), _cuda(c["dy"], offset)
            nan = np.full(shape, np.nan, np.float32)
            y, mu, rsig = ops.group_norm_forward(x, g, b, G, c["eps"], y=_cuda(nan, offset))
            f = _dispatch()
            dx, dgamma, dbeta = ops.group_norm_backward(dy, x, mu, rsig, g, G, dx=_cuda(nan, offset))
            assert mode in f and mode in _dispatch(), (shape, offset, f, _dispatch())
            res.append([t.clone() for t in (y, mu, rsig, dx, dgamma, dbeta)])
        for o, p, q in zip(gr.OUTPUTS, *res):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32)), (shape, o)


@pytest.mark.gpu
def test_autograd_function_returns_the_raw_arrays(ops):
    import torch
    rs = np.random.RandomState(14)
    for shape, G in (((8, 64, 7, 7), 32), ((2, 64, 100, 168), 32)):
        c = gr.make_case(rs, shape, G, "random", 0.0, 1e-5)
        x = _cuda(c["x"]).requires_grad_()
        g, b = _cuda(c["gamma"]).requires_grad_(), _cuda(c["beta"]).requires_grad_()
        dy = _cuda(c["dy"])
        y, mu, rsig = ops.group_norm(x, g, b, num_group=G, eps=1e-5, return_stats=True)
        assert not mu.requires_grad and not rsig.requires_grad
        ry, rmu, rrsig = ops.group_norm_forward(x.detach(), g.detach(), b.detach(), G, 1e-5)
        assert torch.equal(y.detach(), ry) and torch.equal(mu, rmu) and torch.equal(rsig, rrsig)
        dx, dgamma, dbeta = torch.autograd.grad(y, (x, g, b), dy)
        rdx, rdg, rdb = ops.group_norm_backward(dy, x.detach(), rmu, rrsig, g.detach(), G)
        assert torch.equal(dx, rdx) and torch.equal(dgamma, rdg) and torch.equal(dbeta, rdb)
        only_y = ops.group_norm(x, g, b, num_group=G)
        assert torch.equal(only_y.detach(), ry)
        dx2, = torch.autograd.grad(only_y, (x,), dy)        # data gradient alone: dgamma / dbeta are skipped
        assert torch.equal(dx2, rdx)
