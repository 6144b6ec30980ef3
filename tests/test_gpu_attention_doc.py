"""GPU numerics of the per-document causal mask (``DocMask``): the DOC forms of
forward variant 4 and backward variant 5 (``mxk_attn_fwd_doc`` /
``mxk_attn_bwd_doc``) against the fp32 reference ``attention_ref(doc=...)``,
through the op, the model and the trainer.

Tolerances are those of tests/test_gpu_attention.py: o within 2e-2, lse within
atol 1e-3 / rtol 1e-4, each gradient within 3e-2 * max(1, |want|max)."""
import math
import types

import pytest
import torch

from mxk8s.ops import attention as A
from mxk8s.ops.attention import DocMask

pytestmark = pytest.mark.gpu

D = 128
SHAPES = [(2, 256, 4, 2), (1, 384, 8, 2), (1, 256, 4, 4)]   # the last: grp = 1


def _lengths(starts, S):
    return [b - a for a, b in zip(starts, list(starts[1:]) + [S])]


def _mid(S):
    return [0, 1, 37, 100, 129, 200, S - 1]     # a one-token document at both ends


def _layout(name, B, S):
    """Document starts per batch row (different per row where B = 2)."""
    rows = {
        "single": [[0], [0]],
        "aligned": [[0, 64, 128, 192], [0, 128, 192]],
        "midtile": [_mid(S), [0, 63, 65, 127, 128, S - 2]],
        # rows 100-127 share a wave with rows 96-99, which see tile 0: every
        # key of tile 0 is masked for them; with a start at 96 the whole wave
        # skips tile 0 while its neighbours do not
        "masked_first": [[0, 100], [0, 96]],
        "every": [list(range(S)), list(range(S))],
        "mixed": [[0], _mid(S)],
    }[name]
    return rows[:B]


def _doc(name, B, S, dev):
    return DocMask.from_lengths([_lengths(r, S) for r in _layout(name, B, S)], S, device=dev)


def _inputs(B, S, Hq, Hkv, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    mk = lambda h: torch.randn(B, S, h, D, device=dev, generator=g).bfloat16()  # noqa: E731
    return mk(Hq), mk(Hkv), mk(Hkv), mk(Hq)       # q, k, v, dout


def _run(q, k, v, dout, doc, **kw):
    o, lse = A.attn_fwd(q, k, v, doc=doc)
    dq, dk, dv = A.attn_bwd(q, k, v, o, lse, dout, doc=doc, **kw)
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


_REF = {}


def _reference(shape, name, dev):
    """fp32 reference of one (shape, layout), computed once and shared."""
    if (shape, name) not in _REF:
        B, S, Hq, Hkv = shape
        q, k, v, dout = _inputs(B, S, Hq, Hkv, dev)
        doc = _doc(name, B, S, dev)
        qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
        ref = A.attention_ref(qr, kr, vr, doc=doc)
        ref.backward(dout.float())
        s = qr.detach().transpose(1, 2) @ kr.detach().transpose(1, 2).repeat_interleave(
            Hq // Hkv, dim=1).transpose(-1, -2) / math.sqrt(D)
        s = s.masked_fill(~doc.bool_mask()[:, None], float("-inf"))
        _REF[shape, name] = {"o": ref.detach(), "lse": torch.logsumexp(s, dim=-1),
                             "dq": qr.grad, "dk": kr.grad, "dv": vr.grad}
    return _REF[shape, name]


def _assert_close(got, want):
    for name, t in got.items():
        assert torch.isfinite(t.float()).all(), f"{name} has a non-finite value"
    err = (got["o"].float() - want["o"]).abs().max().item()
    print(f"o err {err:.3e}")
    assert err < 2e-2, err
    print(f"lse err {(got['lse'] - want['lse']).abs().max().item():.3e}")
    assert torch.allclose(got["lse"], want["lse"], atol=1e-3, rtol=1e-4)
    for name in ("dq", "dk", "dv"):
        err = (got[name].float() - want[name]).abs().max().item()
        tol = 3e-2 * max(1.0, want[name].abs().max().item())
        print(f"{name} err {err:.3e} tol {tol:.3e}")
        assert err < tol, (name, err, tol)


CASES = [(s, n) for s in SHAPES for n in ("single", "aligned", "midtile", "masked_first", "every")]
CASES.append((SHAPES[0], "mixed"))      # two rows in one launch


@pytest.mark.parametrize("shape,name", CASES, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else x)
def test_doc_attention_matches_reference(cuda_device, shape, name):
    B, S, Hq, Hkv = shape
    q, k, v, dout = _inputs(B, S, Hq, Hkv, cuda_device)
    got = _run(q, k, v, dout, _doc(name, B, S, cuda_device))
    _assert_close(got, _reference(shape, name, cuda_device))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda x: "x".join(map(str, x)))
def test_single_document_is_the_causal_kernels_bit_for_bit(cuda_device, shape):
    """One document: no mask fires and the loop bounds are the causal ones, so
    any difference from forward variant 4 / backward variant 5 is a change to
    the shared math."""
    B, S, Hq, Hkv = shape
    q, k, v, dout = _inputs(B, S, Hq, Hkv, cuda_device)
    got = _run(q, k, v, dout, _doc("single", B, S, cuda_device))
    o, lse = A.attn_fwd(q, k, v, causal=True, variant=4)
    dq, dk, dv = A.attn_bwd(q, k, v, o, lse, dout, causal=True, variant=5)
    for name, want in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.equal(got[name], want), name


@pytest.mark.parametrize("shape", SHAPES, ids=lambda x: "x".join(map(str, x)))
def test_every_token_its_own_document(cuda_device, shape):
    B, S, Hq, Hkv = shape
    grp = Hq // Hkv
    q, k, v, dout = _inputs(B, S, Hq, Hkv, cuda_device)
    got = _run(q, k, v, dout, _doc("every", B, S, cuda_device))
    assert torch.equal(got["o"], v.repeat_interleave(grp, dim=2))
    qk = (q.float() * k.float().repeat_interleave(grp, dim=2)).sum(-1) / math.sqrt(D)   # [B, S, Hq]
    assert torch.allclose(got["lse"], qk.transpose(1, 2), atol=1e-3, rtol=1e-4)
    for name in ("dq", "dk"):
        err = got[name].float().abs().max().item()
        print(f"{name} max {err:.3e}")
        assert err < 3e-2, (name, err)
    want = dout.float().view(B, S, Hkv, grp, D).sum(3)
    err = (got["dv"].float() - want).abs().max().item()
    assert err < 3e-2 * max(1.0, want.abs().max().item()), err


def test_isolation_bit_for_bit(cuda_device):
    """Other documents' q / k / v / dout do not reach a document's rows by a bit."""
    B, S, Hq, Hkv = SHAPES[0]
    q, k, v, dout = _inputs(B, S, Hq, Hkv, cuda_device)
    doc = _doc("midtile", B, S, cuda_device)
    base = _run(q, k, v, dout, doc)
    starts = _layout("midtile", B, S)[0]
    for n, (lo, hi) in enumerate(zip(starts, starts[1:] + [S])):
        other = _inputs(B, S, Hq, Hkv, cuda_device, seed=100 + n)
        mixed = []
        for t, r in zip((q, k, v, dout), other):
            r = r.clone()
            r[0, lo:hi] = t[0, lo:hi]
            mixed.append(r)
        got = _run(*mixed, doc)
        for name in ("o", "dq", "dk", "dv"):
            assert torch.equal(got[name][0, lo:hi], base[name][0, lo:hi]), (name, lo, hi)
        assert torch.equal(got["lse"][0, :, lo:hi], base["lse"][0, :, lo:hi]), ("lse", lo, hi)


def test_run_to_run_identity(cuda_device):
    B, S, Hq, Hkv = SHAPES[1]
    q, k, v, dout = _inputs(B, S, Hq, Hkv, cuda_device)
    doc = _doc("midtile", B, S, cuda_device)
    a, b = _run(q, k, v, dout, doc), _run(q, k, v, dout, doc)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_strided_operands_and_outputs(cuda_device):
    """q / k / v as views of one fused projection buffer, dk / dv as views of a
    fused gradient buffer: the contiguous call's bits, nothing else written."""
    B, S, Hq, Hkv = SHAPES[0]
    q, k, v, dout = _inputs(B, S, Hq, Hkv, cuda_device)
    doc = _doc("midtile", B, S, cuda_device)
    base = _run(q, k, v, dout, doc)
    qkv = torch.cat([t.reshape(B, S, -1) for t in (q, k, v)], dim=-1).contiguous()
    qs, ks, vs = A._split_qkv(qkv, Hq, Hkv, D)
    assert not ks.is_contiguous() and A.supported(qs, ks, vs)
    dqkv = torch.full_like(qkv, float("nan"))
    dqs, dks, dvs = A._split_qkv(dqkv, Hq, Hkv, D)
    got = _run(qs, ks, vs, dout, doc, dk=dks, dv=dvs)
    assert got["dk"] is dks and got["dv"] is dvs
    for name in base:
        assert torch.equal(got[name], base[name]), name
    assert torch.isnan(dqs).all()


def _raw_calls(q, k, v, o, lse, dout, dq, dk, dv, ws, ds_ptr, de_ptr, dev):
    from mxk8s.ops import _lib
    L = _lib.lib()
    B, S, Hq, _ = q.shape
    Hkv = k.shape[2]
    sc = 1.0 / math.sqrt(D)
    st_f = L.mxk_attn_fwd_doc(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(),
                              ds_ptr, B, S, Hq, Hkv, D, q.stride(1), k.stride(1), v.stride(1), sc,
                              _lib.stream_ptr(dev))
    st_b = L.mxk_attn_bwd_doc(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                              dout.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                              dv.data_ptr(), ws.data_ptr(), ds_ptr, de_ptr, B, S, Hq, Hkv, D,
                              q.stride(1), k.stride(1), v.stride(1), dk.stride(1), dv.stride(1), sc,
                              _lib.stream_ptr(dev))
    return st_f, st_b


@pytest.mark.parametrize("why", ["misaligned_doc_start", "S192"])
def test_rejected_before_any_launch(cuda_device, why):
    from mxk8s.ops import _lib
    B, Hq, Hkv = 1, 4, 2
    S = 192 if why == "S192" else 256
    q, k, v, dout = _inputs(B, S, Hq, Hkv, cuda_device)
    doc = DocMask.from_lengths([[S]], S, device=cuda_device)
    sent = 7.0
    o, dq = torch.full_like(q, sent), torch.full_like(q, sent)
    dk, dv = torch.full_like(k, sent), torch.full_like(v, sent)
    lse = torch.full((B, Hq, S), sent, device=cuda_device)
    ws = torch.full((max(1, _lib.lib().mxk_attn_bwd_doc_workspace(B, S, Hq) // 4),), sent,
                    device=cuda_device)
    ds_ptr = doc.doc_start.data_ptr() + (2 if why == "misaligned_doc_start" else 0)
    st = _raw_calls(q, k, v, o, lse, dout, dq, dk, dv, ws, ds_ptr, doc.doc_end.data_ptr(),
                    cuda_device)
    torch.cuda.synchronize()
    assert st == (1, 1), st
    for t in (o, dq, dk, dv, lse, ws):
        assert (t.float() == sent).all()


MODEL_STARTS = [[0, 1, 37, 64, 100], [0, 63, 65, 127]]


def test_tiny_llama_with_mask_matches_cpu_fp32(cuda_device, monkeypatch):
    from mxk8s.models.llama import Llama, LlamaConfig
    from mxk8s.ops import _lib
    L = _lib.lib()
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = L.mxk_attn_fwd_doc, L.mxk_attn_bwd_doc

    def count(name, fn):
        def wrapper(*a):
            calls[name] += 1
            return fn(*a)
        return wrapper
    monkeypatch.setattr(L, "mxk_attn_fwd_doc", count("fwd", fwd))
    monkeypatch.setattr(L, "mxk_attn_bwd_doc", count("bwd", bwd))
    torch.manual_seed(0)
    cfg = LlamaConfig.tiny()
    ref = Llama(cfg)
    gpu = Llama(cfg)
    gpu.load_state_dict(ref.state_dict())
    gpu = gpu.to(cuda_device, torch.bfloat16)
    S = 128
    tok = torch.randint(0, cfg.vocab_size, (2, S + 1))
    doc = DocMask.from_lengths([_lengths(r, S) for r in MODEL_STARTS], S)
    lr = ref.loss(tok, doc=doc)
    lg = gpu.loss(tok.to(cuda_device), doc=doc.to(cuda_device))
    assert calls["fwd"] == cfg.n_layers, calls      # no fall-through to the unmasked kernels
    assert abs(lr.item() - lg.item()) < 0.05, (lr.item(), lg.item())
    lr.backward()
    lg.backward()
    assert calls["bwd"] == cfg.n_layers, calls
    for (n, pr), (_, pg) in zip(ref.named_parameters(), gpu.named_parameters()):
        a, b = pr.grad.float(), pg.grad.float().cpu()
        rel = ((a - b).norm() / (a.norm() + 1e-12)).item()
        assert rel < 0.08, (n, rel)


def test_ddp_bench_tiny_with_doc_len(cuda_device):
    from mxk8s.train.ddp_llama import run_ddp_bench
    a = types.SimpleNamespace(steps=3, warmup=1, seq_len=128, micro_batch=2, layers=None, tiny=True,
                              bucket_mb=1.0, doc_len=32)
    out = run_ddp_bench(a)
    assert out["doc_mask"]["mean_doc_len"] == 32
    assert 0.0 < out["doc_mask"]["visible_fraction"] < 1.0
    assert len(out["losses"]) == 3 and all(math.isfinite(x) for x in out["losses"])
