"""Batched two-view verification on the GPU (sift_hip_verify_fundamental_batched_* / _homography_batched_*; the batched
instantiations of the kernels in csrc/verify.hip), both models.

The bar: pair p's result record, mask, out rows and out_count equal sift_amd.cv.ransac_fundamental / ransac_homography
of that pair's counted records with the seed (seed + p) mod 2^32, as raw bytes, and equal the single-pair device call
on the same verifier; nothing else is written.  The inputs are tests/verify_batched_cases.py;
tests/test_verify_batched_cases.py checks on the CPU that they can tell a pair mix-up, a wrong row offset and an
ignored pair index apart.
"""
import ctypes

import numpy as np
import pytest

import epipolar_cases as ec
import homography_cases as hc
import verify_batched_cases as bc

pytestmark = pytest.mark.gpu
FILL = 0x5A  # the outputs start as this byte: what the device does not write stays visible
GUARD = 96   # rows / entries behind the batch's own that must keep the fill
STATE = -3   # SIFT_HIP_ERR_STATE
BATCHES = ("MIXED", "LARGE64", "FULL")


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


def dtype_of(sift, model):
    return sift.VERIFY_RESULT_DTYPE if model == "fundamental" else sift.HOMOGRAPHY_RESULT_DTYPE


class Inputs:
    """A batch on the device: the match rows, the counters, every pair's positions at the given strides (an empty pair
    gets null pointers and no rows)."""

    def __init__(self, sift, model, batch, stride=(2, 2)):
        self.sift, self.model, self.batch, self.stride = sift, model, batch, stride
        self.K, self.seed = bc.BATCHES[batch]
        self.host = bc.pairs(model, batch)
        self.caps, self.row0 = bc.caps(model, batch), bc.row0(model, batch)
        self.P, self.rows = len(self.host), int(self.row0[-1])
        self.dm = dev(sift, bc.matches(model, batch))
        self.dc = dev(sift, bc.counts(model, batch))
        self.dxy = [(dev(sift, ec.with_stride(p["q_xy"], stride[0])), dev(sift, ec.with_stride(p["t_xy"], stride[1])))
                    if len(p["buf"]) else None for p in self.host]
        self.pairs = [(d[0].value, len(p["q_xy"]), d[1].value, len(p["t_xy"]), cap) if d else (0, 0, 0, 0, 0)
                      for p, d, cap in zip(self.host, self.dxy, self.caps)]


class Outputs:
    """Results, out rows, out counts and masks of P pairs over `rows` rows, prefilled, with a guard behind each."""

    def __init__(self, sift, model, P, rows):
        self.sift, self.model, self.P, self.rows = sift, model, P, rows
        self.res = dev(sift, np.full(52 * (P + 1), FILL, np.uint8))
        self.out = dev(sift, np.full(16 * (rows + GUARD), FILL, np.uint8))
        self.cnt = dev(sift, np.full(4 * (P + 1), FILL, np.uint8))
        self.mask = dev(sift, np.full(rows + GUARD, FILL, np.uint8))

    def read(self):
        s = self.sift
        return dict(results=self.res.to_numpy(dtype_of(s, self.model), (self.P + 1,)),
                    out=self.out.to_numpy(s.DMATCH_DTYPE, (self.rows + GUARD,)),
                    out_counts=self.cnt.to_numpy(np.int32, (self.P + 1,)),
                    mask=self.mask.to_numpy(np.uint8, (self.rows + GUARD,)))

    def untouched(self):
        return all((a.view(np.uint8) == FILL).all() for a in self.read().values())


def batched(v, model):
    return v.verify_batched_device if model == "fundamental" else v.verify_homography_batched_device


def single(v, model):
    return v.verify_device if model == "fundamental" else v.verify_homography_device


def run(inp, v, counted=True, stream=None, outputs=None):
    """One batched device call on fresh (or the given) outputs; the outputs on the host."""
    sift = inp.sift
    o = outputs or Outputs(sift, inp.model, inp.P, inp.rows)
    batched(v, inp.model)(inp.dm.value, inp.dc.value if counted else 0, inp.pairs, o.res.value, o.out.value, o.cnt.value,
                          o.mask.value, bc.MAX_ERROR, inp.K, inp.seed, inp.stride[0], inp.stride[1],
                          stream.cuda_stream if stream else None)
    if stream:
        stream.synchronize()
    else:
        sift.lib().sift_hip_device_sync()
    return o.read()


def check_against_the_rule(inp, got, counted=True):
    """Every pair's outputs against the numpy rule with seed + p; the rows behind a pair's list, the guards."""
    field = "F" if inp.model == "fundamental" else "H"
    for p in range(inp.P):
        ref = bc.reference(inp.model, inp.batch, p, counted)
        r, a, cap, n = got["results"][p], inp.row0[p], inp.caps[p], ref["matches"]
        assert r[field].tobytes() == bc.model_of(inp.model, ref).tobytes(), p
        assert (r["inliers"], r["hypothesis"], r["matches"], r["valid_hypotheses"]) == \
            (ref["inliers"], ref["hypothesis"], n, ref["valid_hypotheses"]), p
        assert got["out_counts"][p] == ref["inliers"], p
        rows = got["out"][a:a + cap]
        assert rows[:ref["inliers"]].tobytes() == ref["list"].tobytes(), p
        assert rows[:ref["inliers"]].tobytes() == inp.host[p]["buf"][:n][ref["mask"] != 0].tobytes(), p
        assert (rows[ref["inliers"]:].view(np.uint8) == FILL).all(), p  # rows past the pair's list keep the fill
        mask = got["mask"][a:a + cap]
        assert np.array_equal(mask[:n], ref["mask"]) and not mask[n:].any(), p  # all cap bytes are written
    assert (got["results"][inp.P:].view(np.uint8) == FILL).all() and (got["out_counts"][inp.P:].view(np.uint8) == FILL).all()
    assert (got["out"][inp.rows:].view(np.uint8) == FILL).all() and (got["mask"][inp.rows:] == FILL).all()


def singles(inp, v, counted=True):
    """The same pairs through P single-pair device calls on the same verifier, seed + p each, laid out as a batch."""
    sift = inp.sift
    o = Outputs(sift, inp.model, inp.P, inp.rows)
    for p, (q, nq, t, nt, cap) in enumerate(inp.pairs):
        a = int(inp.row0[p])
        single(v, inp.model)(inp.dm.value + 16 * a if cap else 0, inp.dc.value + 4 * p if counted else 0, cap, q, nq, t, nt,
                             o.res.value + 52 * p, o.out.value + 16 * a, o.cnt.value + 4 * p, o.mask.value + a, bc.MAX_ERROR,
                             inp.K, (inp.seed + p) % bc.U32, inp.stride[0], inp.stride[1])
    sift.lib().sift_hip_device_sync()
    return o.read()


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.fixture(scope="module")
def verifier(sift):
    """One verifier for the module: 64 pairs, MIXED's rows and K.  Sharing it is part of the test (scratch reuse)."""
    rows = max(int(bc.row0(m, b)[-1]) for m in bc.MODELS for b in BATCHES)
    return sift.Verifier(rows, 256, 64)


@pytest.mark.parametrize("counted", [True, False], ids=["device_counts", "null_counts"])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("model", bc.MODELS)
def test_every_pair_equals_the_rule_and_the_single_call(sift, verifier, model, batch, counted):
    inp = Inputs(sift, model, batch)
    got = run(inp, verifier, counted)
    check_against_the_rule(inp, got, counted)
    assert same_bytes(got, singles(inp, verifier, counted))


@pytest.mark.parametrize("model", bc.MODELS)
def test_two_runs_scratch_reuse_and_another_stream(sift, verifier, model):
    import torch

    mixed, full = Inputs(sift, model, "MIXED"), Inputs(sift, model, "FULL")
    a = run(mixed, verifier)
    b = run(mixed, verifier)
    assert same_bytes(a, b)
    check_against_the_rule(full, run(full, verifier))
    c = run(mixed, verifier)  # after FULL's 64 pairs on the same scratch: nothing stale leaks
    check_against_the_rule(mixed, c)
    assert same_bytes(a, c)
    s = torch.cuda.Stream()
    check_against_the_rule(full, run(full, verifier, stream=s))
    d = run(mixed, verifier, stream=s)
    check_against_the_rule(mixed, d)
    assert same_bytes(a, d)


@pytest.mark.parametrize("strides", [(2, 2), (3, 3), (5, 2)])
@pytest.mark.parametrize("model", bc.MODELS)
def test_strides_give_identical_results(sift, verifier, model, strides):
    inp = Inputs(sift, model, "MIXED", strides)
    check_against_the_rule(inp, run(inp, verifier))


@pytest.mark.parametrize("model", bc.MODELS)
def test_one_pair_on_a_plain_verifier_and_refusals(sift, model):
    inp = Inputs(sift, model, "LARGE64")
    small, large = inp.pairs
    v = sift.Verifier(inp.rows, inp.K)  # the plain creation: max_pairs = 1
    assert v.max_pairs == 1
    one = Inputs(sift, model, "LARGE64")
    one.P, one.rows, one.pairs, one.caps, one.host = 1, inp.caps[0], [small], inp.caps[:1], inp.host[:1]
    got = run(one, v)
    check_against_the_rule(one, got)
    assert same_bytes(got, singles(one, v))
    o = Outputs(sift, model, 65, inp.rows)
    call = lambda pairs, **kw: batched(v, model)(inp.dm.value, 0, pairs, o.res.value, o.out.value, o.cnt.value,  # noqa: E731
                                                 o.mask.value, bc.MAX_ERROR, kw.get("K", inp.K), 0, 2, 2)
    with pytest.raises(sift.SiftHipError, match="max_pairs"):
        call([small, large])
    with pytest.raises(sift.SiftHipError, match="pairs outside"):
        call([small] * 65)
    with pytest.raises(sift.SiftHipError, match="cap must lie"):
        call([small[:4] + (65537,)])
    with pytest.raises(sift.SiftHipError, match="max_matches"):
        call([large[:4] + (inp.rows + 1,)])
    with pytest.raises(sift.SiftHipError, match="hypotheses"):
        call([small], K=inp.K + 1)
    many = sift.Verifier(inp.rows, inp.K, 2)
    with pytest.raises(sift.SiftHipError, match="max_matches"):  # the caps' sum, each cap in range
        batched(many, model)(inp.dm.value, 0, [large, large], o.res.value, o.out.value, o.cnt.value, o.mask.value,
                             bc.MAX_ERROR, inp.K, 0, 2, 2)
    with pytest.raises(sift.SiftHipError, match="max_pairs"):
        batched(many, model)(inp.dm.value, 0, [small] * 3, o.res.value, o.out.value, o.cnt.value, o.mask.value,
                             bc.MAX_ERROR, inp.K, 0, 2, 2)
    with pytest.raises(sift.SiftHipError, match="alias"):
        batched(many, model)(inp.dm.value, 0, [small, large], o.res.value, inp.dm.value + 16 * (inp.rows - 1), o.cnt.value,
                             o.mask.value, bc.MAX_ERROR, inp.K, 0, 2, 2)
    sift.lib().sift_hip_device_sync()
    assert o.untouched()  # nothing was launched
    spill = sift.Verifier(bc.SPILL["max_matches"], 64, 2)  # SPILL: refused for the cap of 70 000, never run
    with pytest.raises(sift.SiftHipError, match="cap must lie"):
        batched(spill, model)(inp.dm.value, 0, [small[:4] + (c,) for c in bc.SPILL["caps"]], o.res.value, 0, 0, 0,
                              bc.MAX_ERROR, 64, 0, 2, 2)
    sift.lib().sift_hip_device_sync()
    assert o.untouched()


def test_getters_after_a_batched_call(sift, verifier):
    L = sift.lib()
    getters = {"fundamental": L.sift_hip_verify_hypotheses_host, "homography": L.sift_hip_verify_homography_hypotheses_host}
    for model in bc.MODELS:
        inp = Inputs(sift, model, "LARGE64")
        run(inp, verifier)
        for g in getters.values():
            assert g(verifier._v, None, None, None, 4) == STATE
            assert b"batch" in L.sift_hip_last_error()
        with pytest.raises(sift.SiftHipError, match="batch"):
            verifier.hypotheses()
        with pytest.raises(sift.SiftHipError, match="batch"):
            verifier.homography_hypotheses()
        # a following single call: its own getter answers again, with that call's hypotheses
        q, nq, t, nt, cap = inp.pairs[0]
        res = dev(sift, np.zeros(52, np.uint8))
        single(verifier, model)(inp.dm.value, 0, cap, q, nq, t, nt, res.value, 0, 0, 0, bc.MAX_ERROR, inp.K, inp.seed, 2, 2)
        samples, M, valid, counts = verifier.hypotheses() if model == "fundamental" else verifier.homography_hypotheses()
        ref = bc.reference(model, "LARGE64", 0)  # pair 0: seed + 0
        assert np.array_equal(samples, ref["samples"]) and np.array_equal(counts, ref["counts"])
        assert M.tobytes() == ref["Fs" if model == "fundamental" else "Hs"].tobytes()
        other = getters["homography" if model == "fundamental" else "fundamental"]
        assert other(verifier._v, None, None, None, 4) == STATE and b"other model" in L.sift_hip_last_error()


def test_chain_on_one_stream(sift):
    """match_list_batched -> verify_homography_batched_device with cap[p] = nq[p] and the list's own device counters, on
    one stream with no host synchronisation between them: equal, byte for byte, to the per-pair chain
    match_list_device -> verify_homography_device with the seed + p, the records carrying imgIdx = p."""
    import torch

    shapes, K, seed = [(65, 64), (48, 56), (80, 72)], 256, 3
    sets = [hc.chain_case(*s) for s in shapes]
    up = lambda rows: dev(sift, rows.astype(np.float16).view(np.uint16))  # noqa: E731
    dq, dt = [up(c[0]) for c in sets], [up(c[1]) for c in sets]
    dqxy, dtxy = [dev(sift, ec.with_stride(c[2], 3)) for c in sets], [dev(sift, ec.with_stride(c[3], 3)) for c in sets]
    nqs, nts, P = [s[0] for s in shapes], [s[1] for s in shapes], len(shapes)
    rows, row0 = sum(nqs), np.concatenate([[0], np.cumsum(nqs)]).astype(int)
    m, v = sift.Matcher(max(nqs + nts), max(nqs + nts), max_pairs=P), sift.Verifier(rows, K, P)
    warm, wcnt = dev(sift, np.zeros(16 * rows, np.uint8)), dev(sift, np.zeros(4 * P, np.uint8))
    qp, tp = [d.value for d in dq], [d.value for d in dt]
    m.match_list_batched(qp, nqs, tp, nts, warm.value, wcnt.value)  # the matcher's first list calls allocate
    m.match_list_device(qp[0], nqs[0], tp[0], nts[0], warm.value, wcnt.value)
    sift.lib().sift_hip_device_sync()
    lst, cnt = dev(sift, np.full(16 * rows, FILL, np.uint8)), dev(sift, np.full(4 * P, FILL, np.uint8))
    o = Outputs(sift, "homography", P, rows)
    pairs = [(dqxy[p].value, nqs[p], dtxy[p].value, nts[p]) for p in range(P)]  # cap defaults to nq
    s = torch.cuda.Stream()
    m.match_list_batched(qp, nqs, tp, nts, lst.value, cnt.value, stream=s.cuda_stream)
    v.verify_homography_batched_device(lst.value, cnt.value, pairs, o.res.value, o.out.value, o.cnt.value, o.mask.value,
                                       hc.MAX_ERROR, K, seed, 3, 3, stream=s.cuda_stream)
    s.synchronize()
    got = o.read()
    counts = cnt.to_numpy(np.int32, (P,))
    lists = lst.to_numpy(sift.DMATCH_DTYPE, (rows,))
    v1 = sift.Verifier(max(nqs), K)
    for p in range(P):
        l1, c1 = dev(sift, np.full(16 * nqs[p], FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
        r1, o1 = dev(sift, np.full(52, FILL, np.uint8)), dev(sift, np.full(16 * nqs[p], FILL, np.uint8))
        n1, m1 = dev(sift, np.full(4, FILL, np.uint8)), dev(sift, np.full(nqs[p], FILL, np.uint8))
        m.match_list_device(qp[p], nqs[p], tp[p], nts[p], l1.value, c1.value, stream=s.cuda_stream)
        v1.verify_homography_device(l1.value, c1.value, nqs[p], dqxy[p].value, nqs[p], dtxy[p].value, nts[p], r1.value,
                                    o1.value, n1.value, m1.value, hc.MAX_ERROR, K, seed + p, 3, 3, stream=s.cuda_stream)
        s.synchronize()
        n = int(c1.to_numpy(np.int32, (1,))[0])
        assert n == counts[p] and n >= 8
        want = l1.to_numpy(sift.DMATCH_DTYPE, (nqs[p],))[:n].copy()
        want["imgIdx"] = p
        a = int(row0[p])
        assert lists[a:a + n].tobytes() == want.tobytes()
        r = r1.to_numpy(sift.HOMOGRAPHY_RESULT_DTYPE, (1,))[0]
        assert got["results"][p].tobytes() == r.tobytes() and r["hypothesis"] >= 0 and r["matches"] == n
        k = int(n1.to_numpy(np.int32, (1,))[0])
        assert got["out_counts"][p] == k == r["inliers"] and k >= 4
        inl = o1.to_numpy(sift.DMATCH_DTYPE, (nqs[p],))[:k].copy()
        inl["imgIdx"] = p
        assert got["out"][a:a + k].tobytes() == inl.tobytes() and (got["out"][a:a + k]["imgIdx"] == p).all()
        assert (got["out"][a + k:a + nqs[p]].view(np.uint8) == FILL).all()
        assert got["mask"][a:a + nqs[p]].tobytes() == m1.to_numpy(np.uint8, (nqs[p],)).tobytes()
    assert (got["out"][rows:].view(np.uint8) == FILL).all() and (got["mask"][rows:] == FILL).all()


@pytest.mark.parametrize("model", bc.MODELS)
def test_host_forms_and_module_functions(sift, verifier, model):
    inp = Inputs(sift, model, "MIXED", (3, 3))
    got = run(inp, verifier)
    host = verifier.verify_batched_host if model == "fundamental" else verifier.verify_homography_batched_host
    field = "F" if model == "fundamental" else "H"
    full = host(inp.dm.value, inp.dc.value, inp.pairs, bc.MAX_ERROR, inp.K, inp.seed, 3, 3, full=True)
    short = host(inp.dm.value, inp.dc.value, inp.pairs, bc.MAX_ERROR, inp.K, inp.seed, 3, 3)
    assert len(full) == len(short) == inp.P
    for p in range(inp.P):
        a, cap, k = int(inp.row0[p]), inp.caps[p], int(got["out_counts"][p])
        rec, recs, mask = full[p]
        assert rec.tobytes() == got["results"][p].tobytes()
        assert recs.tobytes() == got["out"][a:a + k].tobytes() and mask.tobytes() == got["mask"][a:a + cap].tobytes()
        M, recs2, hyp = short[p]
        assert M.dtype == np.float32 and M.shape == (3, 3) and M.tobytes() == got["results"][p][field].tobytes()
        assert recs2.tobytes() == recs.tobytes() and hyp == got["results"][p]["hypothesis"]
    # the module-level functions take host arrays and count every record they are given: the lists that count
    fn = sift.verifyFundamentalBatched if model == "fundamental" else sift.verifyHomographyBatched
    lists = [p["buf"][:p["count"]] for p in inp.host]
    xy = [(p["q_xy"], p["t_xy"]) for p in inp.host]
    once = fn(lists, xy, bc.MAX_ERROR, inp.K, inp.seed)
    assert len(once) == inp.P
    for p in range(inp.P):
        M, recs, hyp = once[p]
        assert M.tobytes() == short[p][0].tobytes() and recs.tobytes() == short[p][1].tobytes() and hyp == short[p][2]
    with pytest.raises(ValueError):
        fn(lists, xy[:-1])
    assert ctypes.sizeof(sift._VerifyPair) == 32
