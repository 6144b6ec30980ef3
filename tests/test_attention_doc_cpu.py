"""Per-document causal mask on the CPU: the ``DocMask`` constructors, the fp32
reference, the model ("packed equals alone"), argument errors, the trainer's
seeded tables, the library declarations and the host program of the tile
bounds (native/kernels/tests/attention_doc_sweep.cc)."""
import math
import os
import subprocess
import types

import pytest
import torch

from mxk8s.ops import attention as A
from mxk8s.ops.attention import DocMask

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hand-written layouts: document starts per row, S = 16
S16 = 16
STARTS = [[0, 1, 5, 8, 15], [0, 7, 9]]


def _tables(starts, S):
    ds, de = [], []
    for row in starts:
        s_row, e_row = [0] * S, [0] * S
        for lo, hi in zip(row, row[1:] + [S]):
            for i in range(lo, hi):
                s_row[i], e_row[i] = lo, hi
        ds.append(s_row)
        de.append(e_row)
    return torch.tensor(ds, dtype=torch.int32), torch.tensor(de, dtype=torch.int32)


def _lengths(row, S):
    return [b - a for a, b in zip(row, row[1:] + [S])]


def test_constructors_agree_on_hand_written_layouts():
    ds, de = _tables(STARTS, S16)
    a = DocMask.from_lengths([_lengths(r, S16) for r in STARTS], S16)
    ids = torch.zeros(2, S16, dtype=torch.long)
    tokens = torch.full((2, S16), 5)
    for b, row in enumerate(STARTS):
        for n, lo in enumerate(row):
            ids[b, lo:] = 10 * n + b
            if lo:
                tokens[b, lo - 1] = 2        # the previous document ends with eos
    tokens[0, S16 - 1] = 2                   # an eos on the last column opens nothing
    for m in (a, DocMask.from_ids(ids), DocMask.from_eos(tokens, 2), DocMask.from_doc_start(ds),
              DocMask.from_doc_start(ds.long()), a.to("cpu")):
        assert m.doc_start.dtype == torch.int32 and m.doc_end.dtype == torch.int32
        assert m.doc_start.is_contiguous() and m.shape == (2, S16)
        assert torch.equal(m.doc_start, ds)
        assert torch.equal(m.doc_end, de)
    with pytest.raises(AttributeError):
        a.doc_start = ds
    with pytest.raises(TypeError):
        DocMask(ds, de)
    with pytest.raises(ValueError):
        DocMask.from_lengths([[8, 7]], S16)
    with pytest.raises(ValueError):
        DocMask.from_lengths([[16, 0]], S16)


@pytest.mark.parametrize("bad", [
    [1, 1, 1, 1],        # doc_start[0] != 0
    [0, 0, 3, 3],        # a value greater than i
    [0, 1, 0, 0],        # a decrease
    [0, 0, 1, 1],        # a jump to something other than i
])
def test_from_doc_start_rejects_invalid_tables(bad):
    with pytest.raises(ValueError):
        DocMask.from_doc_start(torch.tensor([[0, 0, 2, 2], bad]))
    DocMask.from_doc_start(torch.tensor([[0, 0, 2, 2], [0, 1, 2, 2]]))


def test_visible_fraction_equals_a_brute_force_count():
    m = DocMask.from_lengths([_lengths(r, S16) for r in STARTS], S16)
    ds = m.doc_start.tolist()
    n = sum(1 for b in range(2) for i in range(S16) for j in range(S16) if ds[b][i] <= j <= i)
    assert m.visible_fraction() == pytest.approx(n / (2 * S16 * (S16 + 1) / 2), rel=1e-12)
    assert isinstance(m.visible_fraction(), float)
    assert DocMask.from_lengths([[S16]], S16).visible_fraction() == 1.0
    assert int(m.bool_mask().sum()) == n


def _qkv(B, S, Hq, Hkv, D=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, Hq, D, generator=g), torch.randn(B, S, Hkv, D, generator=g),
            torch.randn(B, S, Hkv, D, generator=g))


def test_attention_ref_with_mask_equals_brute_force():
    B, Hq, Hkv, D = 2, 4, 2, 16
    q, k, v = _qkv(B, S16, Hq, Hkv, D)
    m = DocMask.from_lengths([_lengths(r, S16) for r in STARTS], S16)
    got = A.attention_ref(q, k, v, doc=m)
    ds = m.doc_start.tolist()
    want = torch.zeros_like(got)
    for b in range(B):
        for h in range(Hq):
            for i in range(S16):
                keys = list(range(ds[b][i], i + 1))
                s = torch.stack([q[b, i, h] @ k[b, j, h // (Hq // Hkv)] for j in keys]) / math.sqrt(D)
                p = torch.softmax(s, dim=0)
                want[b, i, h] = sum(p[n] * v[b, j, h // (Hq // Hkv)] for n, j in enumerate(keys))
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5)
    one = DocMask.from_lengths([[S16], [S16]], S16)
    assert torch.equal(A.attention_ref(q, k, v, doc=one), A.attention_ref(q, k, v, causal=True))
    assert torch.equal(A.flash_attention(q, k, v, doc=m), got)       # CPU: the reference


def test_flash_attention_argument_errors():
    q, k, v = _qkv(2, S16, 4, 2)
    m = DocMask.from_lengths([_lengths(r, S16) for r in STARTS], S16)
    with pytest.raises(ValueError):
        A.flash_attention(q, k, v, causal=False, doc=m)              # full attention with doc
    with pytest.raises(ValueError):
        A.flash_attention(q[:1], k[:1], v[:1], doc=m)                # [B, S] mismatch
    with pytest.raises(ValueError):
        A.flash_attention(q[:, :8], k[:, :8], v[:, :8], doc=m)
    with pytest.raises(ValueError):
        A.flash_attention(q.to("meta"), k.to("meta"), v.to("meta"), doc=m)   # device mismatch
    with pytest.raises(ValueError):
        A.attn_fwd(q, k, v, variant=4, doc=m)
    with pytest.raises(ValueError):
        A.attn_bwd(q, k, v, q, q, q, variant=5, doc=m)


MODEL_STARTS = [[0, 1, 37, 64, 100], [0, 63, 65, 127]]


def test_packed_equals_alone():
    """The logits of every document inside a packed row equal the logits of
    that document run alone: positions are not reset, and RoPE is relative.
    Measured with a reference mask: max difference 1.5e-6 on logits of
    magnitude 2; atol 5e-5 is about 30x that."""
    from mxk8s.models.llama import Llama, LlamaConfig
    torch.manual_seed(0)
    S = 128
    model = Llama(LlamaConfig.tiny())
    tok = torch.randint(0, model.cfg.vocab_size, (2, S))
    doc = DocMask.from_lengths([_lengths(r, S) for r in MODEL_STARTS], S)
    with torch.no_grad():
        packed = model(tok, doc=doc)
        unmasked = model(tok)
        worst = 0.0
        for b, row in enumerate(MODEL_STARTS):
            for lo, hi in zip(row, row[1:] + [S]):
                alone = model(tok[b:b + 1, lo:hi])
                worst = max(worst, (packed[b, lo:hi] - alone[0]).abs().max().item())
                assert torch.allclose(packed[b, lo:hi], alone[0], atol=5e-5, rtol=0), (b, lo, hi)
    print(f"packed vs alone: max difference {worst:.3e}")
    assert not torch.allclose(packed, unmasked, atol=1e-3)     # the mask does something
    with pytest.raises(ValueError):
        model(tok[:, :64], doc=doc)


def test_loss_takes_the_mask_of_its_input_columns():
    from mxk8s.models.llama import Llama, LlamaConfig
    torch.manual_seed(0)
    S = 128
    model = Llama(LlamaConfig.tiny())
    tok = torch.randint(0, model.cfg.vocab_size, (2, S + 1))
    doc = DocMask.from_lengths([_lengths(r, S) for r in MODEL_STARTS], S)
    with torch.no_grad():
        a = model.loss(tok, doc=doc)
        b = model.loss(tok[:, :-1], tok[:, 1:], doc=doc)
    assert torch.isfinite(a) and torch.equal(a, b)


def test_flops_per_token_scales_the_attention_term():
    from mxk8s.models.llama import LlamaConfig
    cfg = LlamaConfig.tiny()
    full = cfg.flops_per_token(128)
    assert cfg.flops_per_token(128, None) == full and cfg.flops_per_token(128, 1.0) == full
    attn = 6 * cfg.n_layers * cfg.dim * 128
    assert cfg.flops_per_token(128, 0.25) == pytest.approx(full - 0.75 * attn)


def test_trainer_tables_are_seeded():
    from mxk8s.train.ddp_llama import synthetic_doc_masks
    a = synthetic_doc_masks(4, 2, 128, 32, 2000)
    b = synthetic_doc_masks(4, 2, 128, 32, 2000)
    c = synthetic_doc_masks(4, 2, 128, 32, 2001)
    assert len(a) == 4 and all(m.shape == (2, 128) for m in a)
    assert all(torch.equal(x.doc_start, y.doc_start) for x, y in zip(a, b))
    assert any(not torch.equal(x.doc_start, y.doc_start) for x, y in zip(a, c))
    for m in a:
        DocMask.from_doc_start(m.doc_start)          # valid by the rule
    assert len({tuple(m.doc_start.flatten().tolist()) for m in a}) > 1
    one = synthetic_doc_masks(1, 1, 64, 1, 0)[0]     # mean 1: every token its own document
    assert one.doc_start[0].tolist() == list(range(64))


def test_run_ddp_bench_with_and_without_doc_len(monkeypatch):
    from mxk8s.train.ddp_llama import run_ddp_bench
    monkeypatch.delenv("MXK_DOC_LEN", raising=False)
    base = dict(steps=2, warmup=1, seq_len=64, micro_batch=2, layers=None, tiny=True, bucket_mb=1.0)
    out = run_ddp_bench(types.SimpleNamespace(**base, doc_len=32))
    assert out["doc_mask"]["mean_doc_len"] == 32
    assert 0.0 < out["doc_mask"]["visible_fraction"] <= 1.0
    assert math.isfinite(out["mean_loss"]) and "documents" in out["data"]
    off = run_ddp_bench(types.SimpleNamespace(**base))
    assert off["doc_mask"] is None and "documents" not in off["data"]
    assert off["mfu"] >= 0
    monkeypatch.setenv("MXK_DOC_LEN", "16")
    env = run_ddp_bench(types.SimpleNamespace(**base))
    assert env["doc_mask"]["mean_doc_len"] == 16


def test_lib_declares_the_new_entry_points():
    from mxk8s.ops import _lib
    for name in ("mxk_attn_fwd_doc", "mxk_attn_bwd_doc_workspace", "mxk_attn_bwd_doc"):
        assert name in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["mxk_attn_fwd_doc"][1]) == 16
    assert len(_lib._SIGNATURES["mxk_attn_bwd_doc_workspace"][1]) == 3
    assert len(_lib._SIGNATURES["mxk_attn_bwd_doc"][1]) == 24


def test_doc_plan_program_passes_under_sanitizers():
    """attn_doc_ok and the tile-bound helpers of attention_plan.h, as a
    stand-alone ASan + UBSan host binary (make test-attention-doc)."""
    r = subprocess.run(["make", "-C", REPO, "test-attention-doc"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ", 0 bad" in r.stdout
