"""GPU checks of the fused top-k search (csrc/search.hip via contrastors_amd.search.FlatIPIndex): accuracy against a float64
scorer on the same bf16 inputs plus a stable sort, determinism across runs and corpus split counts, a corpus past 4 GiB,
the workspace bound, the two data-curation tools end to end, and encode() against the training forward."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
DEV = "cuda:0"


def _unit_bf16(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, d, device=DEV, generator=g)
    return torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)


def ref_topk(Q, D, k, exclude=None, below=None, chunk_elems=1 << 27):
    """float64 scores of the bf16 operands, inadmissible -> dropped, stable sort (descending score, then ascending id);
    padded with (-inf, -1) like the kernel."""
    M, N = Q.shape[0], D.shape[0]
    Qd = Q.double()
    best_s = torch.full((M, 0), -float("inf"), dtype=torch.float64, device=DEV)
    best_i = torch.full((M, 0), -1, dtype=torch.int64, device=DEV)
    ch = max(1, chunk_elems // max(M, 1))
    for c0 in range(0, N, ch):
        c1 = min(N, c0 + ch)
        s = Qd @ D[c0:c1].double().T
        ids = torch.arange(c0, c1, device=DEV).expand(M, -1)
        if below is not None:
            s = torch.where(s < below.double()[:, None], s, torch.full_like(s, -float("inf")))
        if exclude is not None:
            for r, ex in enumerate(exclude):
                ex = [e - c0 for e in ex if c0 <= e < c1]
                if ex:
                    s[r, ex] = -float("inf")
        cs = torch.cat([best_s, s], 1)
        ci = torch.cat([best_i, ids], 1)
        o = torch.sort(ci, dim=1, stable=True).indices      # ascending id first ...
        cs, ci = cs.gather(1, o), ci.gather(1, o)
        o = torch.sort(cs, dim=1, descending=True, stable=True).indices[:, :k]   # ... then descending score, stable
        best_s, best_i = cs.gather(1, o), ci.gather(1, o)
    if best_s.shape[1] < k:
        pad = k - best_s.shape[1]
        best_s = torch.cat([best_s, torch.full((M, pad), -float("inf"), dtype=torch.float64, device=DEV)], 1)
        best_i = torch.cat([best_i, torch.full((M, pad), -1, dtype=torch.int64, device=DEV)], 1)
    best_i = torch.where(torch.isinf(best_s), torch.full_like(best_i, -1), best_i)
    return best_s, best_i


def check_against_ref(Q, D, s, i, k, exclude=None, below=None, ref=None):
    """ref: a precomputed ref_topk(..., k' >= k) (its first k columns are the top-k)."""
    rs, ri = ref_topk(Q, D, k, exclude, below) if ref is None else (ref[0][:, :k], ref[1][:, :k])
    valid_k, valid_r = i >= 0, ri >= 0
    assert torch.equal(valid_k, valid_r), "admissible counts differ"
    assert torch.equal(torch.isinf(s) & (s < 0), ~valid_k)
    # the kernel's own order: non-increasing scores, equal scores by ascending id
    if k > 1:
        a_s, b_s, a_i, b_i = s[:, :-1], s[:, 1:], i[:, :-1], i[:, 1:]
        both = (a_i >= 0) & (b_i >= 0)
        assert bool(((a_s > b_s) | ((a_s == b_s) & (a_i < b_i)) | ~both).all()), "output not in (score desc, id asc) order"
    # scores: positionally within 1e-4 of the float64 top-k, and of the exact score of the id returned
    assert float((s.double() - rs)[valid_k].abs().max()) < 1e-4 if bool(valid_k.any()) else True
    if bool(valid_k.any()):
        rows = torch.arange(Q.shape[0], device=DEV)[:, None].expand_as(i)
        exact = (Q.double()[rows[valid_k]] * D.double()[i[valid_k]]).sum(1)
        assert float((exact - s[valid_k].double()).abs().max()) < 1e-4
    # ids: the sets agree except for entries within 1e-5 of the row's k-th score
    kth = torch.where(valid_r, rs, torch.full_like(rs, float("inf"))).min(1).values
    mism = (i != ri) & valid_k
    for r in torch.nonzero(mism.any(1)).flatten().tolist():
        got, want = set(i[r][i[r] >= 0].tolist()), set(ri[r][ri[r] >= 0].tolist())
        for x in got ^ want:
            sx = float(Q[r].double() @ D[x].double())
            assert abs(sx - float(kth[r])) <= 1e-5, (r, x, sx, float(kth[r]))


def _index(D, **kw):
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(D.shape[1], device=DEV, **kw)
    ix.add(D)
    return ix


@pytest.mark.parametrize("d", [64, 256, 768])
@pytest.mark.parametrize("N", [1, 255, 257, 1_000_003])
@pytest.mark.parametrize("M", [1, 300, 4096])
def test_search_accuracy_grid(M, N, d):
    Q, D = _unit_bf16(M, d, 1000 + M), _unit_bf16(N, d, 2000 + N)
    ix = _index(D)
    ref = ref_topk(Q, D, 1024)
    for k in (1, 2, 100, 1024):
        s, i = ix.search(Q, k)
        assert s.shape == (M, k) and i.shape == (M, k) and s.dtype == torch.float32 and i.dtype == torch.int64
        check_against_ref(Q, D, s, i, k, ref=ref)


def test_search_ties_exclusions_bounds_and_padding():
    d, N, M = 128, 600, 300
    base = _unit_bf16(200, d, 7)
    D = torch.cat([base, base, base])                   # every document three times: exact score ties
    Q = torch.cat([_unit_bf16(M - 4, d, 8), D[[0, 5, 399, 599]]])   # the last queries equal documents
    ix = _index(D)
    for k in (1, 3, 100, 1024):
        s, i = ix.search(Q, k)
        check_against_ref(Q, D, s, i, k)
    s, i = ix.search(Q[-4:], 3)
    assert i[:, 0].tolist() == [0, 5, 199, 199], i          # equal-score copies: the lowest id first
    # exclusions: a few ids per row, one row with everything excluded
    g = np.random.default_rng(3)
    excl = [sorted(g.choice(N, size=int(g.integers(0, 6)), replace=False).tolist()) for _ in range(M)]
    excl[5] = list(range(N))
    s, i = ix.search(Q, 50, exclude=excl)
    check_against_ref(Q, D, s, i, 50, exclude=excl)
    assert (i[5] == -1).all() and torch.isinf(s[5]).all()
    for r in range(M):
        assert not set(i[r].tolist()) & set(excl[r])
    # CSR form gives the same bits
    row_ptr = np.concatenate([[0], np.cumsum([len(e) for e in excl])])
    s2, i2 = ix.search(Q, 50, exclude=(row_ptr, np.concatenate([np.asarray(e, dtype=np.int64) for e in excl])))
    assert torch.equal(s, s2) and torch.equal(i, i2)
    # a bound below every score pads everything; a bound in a wide score gap of every row
    s, i = ix.search(Q, 10, below=torch.full((M,), -2.0))
    assert (i == -1).all() and torch.isinf(s).all()
    D2 = _unit_bf16(N, d, 11)
    ix2 = _index(D2)
    full = (Q.double() @ D2.double().T).sort(1, descending=True).values
    gaps = full[:, :60] - full[:, 1:61]
    j = gaps.argmax(1)
    bel = ((full.gather(1, j[:, None]) + full.gather(1, j[:, None] + 1)) / 2).flatten().float()
    assert float(gaps.max(1).values.min()) > 2e-4
    for k in (1, 40, 1024):
        s, i = ix2.search(Q, k, below=bel, exclude=excl)
        check_against_ref(Q, D2, s, i, k, exclude=excl, below=bel)
        assert bool((s[i >= 0] < bel[:, None].expand_as(s)[i >= 0]).all())
    # k > N and an empty index
    s, i = ix2.search(Q[:3], 1024)
    assert (i[:, N:] == -1).all() and (i[:, :N] >= 0).all()
    from contrastors_amd.search import FlatIPIndex
    e = FlatIPIndex(d, device=DEV)
    s, i = e.search(Q[:2], 4)
    assert (i == -1).all() and torch.isinf(s).all()


def test_search_deterministic_across_runs_and_splits():
    M, N, d = 1000, 300_000, 256
    Q, D = _unit_bf16(M, d, 21), _unit_bf16(N, d, 22)
    D[150000:150100] = D[0:100]                           # exact ties between rows of different splits (nsplit > 1)
    ix = _index(D)
    for k in (2, 100, 1024):
        s0, i0 = ix.search(Q, k)
        s1, i1 = ix.search(Q, k)
        assert torch.equal(s0, s1) and torch.equal(i0, i1)
        for ns in (1, 3, 7, 64):
            s2, i2 = ix.search(Q, k, nsplit=ns)
            assert torch.equal(s0, s2) and torch.equal(i0, i2), (k, ns)
    # the host batching (a small workspace bound forces several query batches) gives the same bits
    small = _index(D, workspace_bytes=16 << 20)
    assert small.batch_rows(M, 1024) < M
    s3, i3 = small.search(Q, 1024)
    assert torch.equal(s0, s3) and torch.equal(i0, i3)


def test_search_corpus_past_4gib_finds_planted_neighbours():
    d = 768
    N = (4 << 30) // (2 * d) + 50_000                     # > 4 GiB of bf16
    from contrastors_amd.search import FlatIPIndex

    ix = FlatIPIndex(d, device=DEV)
    ix.reserve(N)                                          # chunks are appended in place: no copy of the corpus
    store = ix._store
    g = torch.Generator(device=DEV).manual_seed(5)
    for c0 in range(0, N, 1 << 20):
        n = min(1 << 20, N - c0)
        ix.add(torch.nn.functional.normalize(torch.randn(n, d, device=DEV, generator=g), dim=1).to(torch.bfloat16))
    assert ix.ntotal * d * 2 > 4 << 30 and ix._store is store
    planted = torch.arange(N - 128, N, device=DEV)
    Q = ix.vectors[planted].clone()
    s, i = ix.search(Q, 4)
    assert torch.equal(i[:, 0], planted), i[:, 0]
    exact = (Q.float() * Q.float()).sum(1)
    assert float((s[:, 0] - exact).abs().max()) < 1e-4
    del ix


def test_search_memory_bound_8192_by_2m():
    M, N, d, k = 8192, 2_000_000, 64, 100
    Q, D = _unit_bf16(M, d, 31), _unit_bf16(N, d, 32)
    ix = _index(D)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    s, i = ix.search(Q, k)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < 2 << 30, extra                          # the score matrix alone would be 64 GB (fp32)
    rows = torch.arange(0, M, 97, device=DEV)
    check_against_ref(Q[rows], D, s[rows], i[rows], k)


def _fx():
    return json.loads((GOLD / "search_curation.json").read_text())


def _tool(name, *args):
    r = subprocess.run([sys.executable, "-m", f"contrastors_amd.tools.{name}", *args], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def _read_shards(out):
    import gzip

    rows = []
    for p in sorted(Path(out).glob("shard-*.jsonl.gz")):
        with gzip.open(p, "rt") as f:
            rows += [json.loads(line) for line in f]
    return rows


def test_tools_end_to_end_from_npy_match_fixtures(tmp_path):
    fx = _fx()
    # consistency filter
    c = fx["consistency"]
    np.save(tmp_path / "cq.npy", np.asarray(c["q"], np.float32))
    np.save(tmp_path / "cd.npy", np.asarray(c["d"], np.float32))
    (tmp_path / "ids.json").write_text(json.dumps(c["ids"]))
    _tool("consistency_filter", "--output_dir", str(tmp_path / "cf"), "--query_embeddings", str(tmp_path / "cq.npy"),
          "--document_embeddings", str(tmp_path / "cd.npy"), "--ids", str(tmp_path / "ids.json"))
    assert json.loads((tmp_path / "cf" / "ids_to_keep_0.json").read_text()) == c["kept"]
    # get_negatives form
    t = fx["topk"]
    with open(tmp_path / "recs.jsonl", "w") as f:
        for r in t["records"]:
            f.write(json.dumps(r) + "\n")
    np.save(tmp_path / "tq.npy", np.asarray(t["q"], np.float32))
    np.save(tmp_path / "td.npy", np.asarray(t["d"], np.float32))
    _tool("mine_negatives", "--rule", "topk", "--dataset", str(tmp_path / "recs.jsonl"), "--output_dir",
          str(tmp_path / "tk"), "--k", str(t["k"]), "--seed", str(t["seed"]), "--query_embeddings", str(tmp_path / "tq.npy"),
          "--document_embeddings", str(tmp_path / "td.npy"))
    got = _read_shards(tmp_path / "tk")
    for g in got:
        assert g.pop("metadata")["objective"]["triplet"] == [["question", "positive_ctxs", "hard_negative_ctxs"]]
    assert got == t["expected"]
    # margin form over a BEIR directory
    m = fx["margin"]
    beir = tmp_path / "beir"
    (beir / "qrels").mkdir(parents=True)
    (beir / "corpus.jsonl").write_text("".join(json.dumps(x) + "\n" for x in m["corpus"]))
    (beir / "queries.jsonl").write_text("".join(json.dumps(x) + "\n" for x in m["queries"]))
    (beir / "qrels" / "train.tsv").write_text("query-id\tcorpus-id\tscore\n" + "".join(f"{a}\t{b}\t{s}\n" for a, b, s in m["qrels"]))
    np.save(tmp_path / "mq.npy", np.asarray(m["q"], np.float32))
    np.save(tmp_path / "md.npy", np.asarray(m["d"], np.float32))
    _tool("mine_negatives", "--rule", "margin", "--dataset", str(beir), "--output_dir", str(tmp_path / "mg"),
          "--k", str(m["k"]), "--max_negatives", str(m["max_negatives"]), "--margin", str(m["margin"]), "--seed",
          str(m["seed"]), "--query_embeddings", str(tmp_path / "mq.npy"), "--document_embeddings", str(tmp_path / "md.npy"))
    got = _read_shards(tmp_path / "mg")
    for g in got:
        g.pop("metadata")
    assert got == m["expected"]
    # the same rows in another order, named by --query_ids
    qids = [f"q{i}" for i in range(len(m["q"]))]
    perm = np.random.default_rng(1).permutation(len(qids))
    np.save(tmp_path / "mq_perm.npy", np.asarray(m["q"], np.float32)[perm])
    (tmp_path / "qids.json").write_text(json.dumps([qids[j] for j in perm]))
    _tool("mine_negatives", "--rule", "margin", "--dataset", str(beir), "--output_dir", str(tmp_path / "mg2"),
          "--k", str(m["k"]), "--max_negatives", str(m["max_negatives"]), "--margin", str(m["margin"]), "--seed",
          str(m["seed"]), "--query_embeddings", str(tmp_path / "mq_perm.npy"), "--query_ids", str(tmp_path / "qids.json"),
          "--document_embeddings", str(tmp_path / "md.npy"))
    got2 = _read_shards(tmp_path / "mg2")
    for g in got2:
        g.pop("metadata")
    assert got2 == m["expected"]


def test_encode_equals_training_forward_in_eval_mode():
    from types import SimpleNamespace

    from contrastors_amd.biencoder import BiEncoder, BiEncoderConfig
    from contrastors_amd.nomic_bert import NomicBertConfig
    from contrastors_amd.search import encode
    from oracle import encoder_ref
    from oracle.data_fixture import WORDS, ToyTokenizer
    from oracle.make_golden import TINY_NOMIC

    cfg = NomicBertConfig(**{k: v for k, v in TINY_NOMIC.items() if k in NomicBertConfig.__dataclass_fields__})
    model = BiEncoder(BiEncoderConfig(pooling="mean", trunk_config=cfg), device=DEV)
    model.trunk.load_reference_state_dict(encoder_ref.random_state_dict(SimpleNamespace(**TINY_NOMIC), 3))
    rng = np.random.default_rng(0)
    texts = [" ".join(rng.choice(WORDS, int(rng.integers(1, 20)))) for _ in range(37)]
    tok = ToyTokenizer()
    got = encode(model, texts, tok, batch_size=8, max_length=32)
    assert got.shape[0] == 37 and model.training
    model.eval()
    t = tok(texts, padding="max_length", truncation=True, return_tensors="pt", max_length=32)
    want = model(input_ids=t["input_ids"].to(DEV), attention_mask=t["attention_mask"].to(DEV))["embedding"].float()
    model.train()
    assert float((got.norm(dim=1) - 1).abs().max()) < 1e-4
    assert float((got - want).abs().max()) < 2e-3, float((got - want).abs().max())
