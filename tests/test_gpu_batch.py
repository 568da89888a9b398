"""GPU tests of the device-resident dataset (csrc/batch_kernels.hip gcnpt_gather_batch, gcn_over_pruned_trees_amd.dataset): a batch's
loader tensors, word dropout included, written in one launch from token arrays that stay in HBM.  The reference is tests/batch_ref.py, a
NumPy restatement of the loader's assembly (data/loader.py:93-141, 182-186) with the project's counter-based drop decision; every
comparison of ids is bit-exact.  Dataset: 37 sentences at Ts = 45, one of 45 tokens and one of 1."""
import functools

import numpy as np
import pytest
import torch

import batch_ref
from helpers import GRAD_RTOL, cuda_dev, gcn_api, to_dev
from gcn_over_pruned_trees_amd import _lib
from gcn_over_pruned_trees_amd.utils import synthetic

pytestmark = pytest.mark.gpu

S, TS = 37, 45
SENTINEL, MASK_SENTINEL, GUARD = -777, 0xCD, 16            # GUARD elements in front of and behind every raw output (keeps 16-byte alignment)
OUT_IDS = ("words", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos")


@pytest.fixture(scope="module")
def dev():
    return cuda_dev()


@pytest.fixture(scope="module")
def api():
    return gcn_api()


@functools.lru_cache(maxsize=None)
def host_dataset():
    """Shared between the tests: read only."""
    rng = np.random.RandomState(20)
    lens = rng.randint(3, TS + 1, size=S).astype(np.int32)
    lens[[0, 1, 2, 3, 4]] = (45, 1, 31, 32, 44)
    tb = synthetic.random_tree_batch(21, S, TS, lengths=lens)
    live = ~tb["masks"]
    words = rng.randint(2, 500, size=(S, TS)).astype(np.int64)
    words[rng.random_sample((S, TS)) < 0.1] = batch_ref.UNK_ID          # some tokens are UNK already
    ds = dict(words=words * live, pos=rng.randint(1, 47, size=(S, TS)) * live, ner=rng.randint(1, 15, size=(S, TS)) * live,
              deprel=tb["deprel"], head=tb["head"], subj_pos=tb["subj_pos"], obj_pos=tb["obj_pos"], lens=lens,
              labels=rng.randint(0, 5, size=S).astype(np.int64))
    for a in ds.values():
        a.setflags(write=False)
    return ds


def device_dataset(with_ner=True):
    return _device_dataset(bool(with_ner))


@functools.lru_cache(maxsize=None)
def _device_dataset(with_ner):
    from gcn_over_pruned_trees_amd import dataset
    h = host_dataset()
    return dataset.DeviceDataset.build(h["words"], h["pos"], h["ner"] if with_ner else None, h["deprel"].astype(np.int32), torch.from_numpy(h["head"].copy()),
                                       h["subj_pos"].astype(np.int16), h["obj_pos"], h["lens"], h["labels"], cuda_dev())


def host_view(with_ner):
    return host_dataset() if with_ner else dict(host_dataset(), ner=None)


def raw_gather(ds, idx, T, p=0.0, seed=0, seed_dev=None, pos_fill=150):
    """gcnpt_gather_batch into sentinel-filled buffers with guard bands; returns the outputs as NumPy arrays and asserts the guards."""
    dev, B = ds.device, len(idx)
    idx_dev = torch.as_tensor(np.asarray(idx, np.int64), device=dev)

    def buf(n, dtype, fill):
        return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    names = [k for k in OUT_IDS if ds.arrays[k] is not None]
    bufs = {k: buf(B * T, torch.int64, SENTINEL) for k in names}
    bufs.update(masks=buf(B * T, torch.uint8, MASK_SENTINEL), labels=buf(B, torch.int64, SENTINEL), lens=buf(B, torch.int32, SENTINEL),
                status=buf(B, torch.int32, SENTINEL))
    P = lambda k: (bufs[k].data_ptr() + GUARD * bufs[k].element_size()) if k in bufs else None  # noqa: E731
    a = ds.arrays
    _lib.check(_lib.lib().gcnpt_gather_batch(
        _lib.stream(), *(_lib.ptr(a[k]) for k in OUT_IDS), _lib.ptr(ds.lens), _lib.ptr(ds.labels), ds.S, ds.Ts, _lib.ptr(idx_dev), B, T,
        P("words"), P("masks"), P("pos"), P("ner"), P("deprel"), P("head"), P("subj_pos"), P("obj_pos"), P("labels"), P("lens"), P("status"),
        pos_fill, p, seed, _lib.ptr(seed_dev)))
    torch.cuda.synchronize()
    out = {}
    for k, t in bufs.items():
        h = t.cpu().numpy()
        fill = MASK_SENTINEL if k == "masks" else SENTINEL
        assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all(), "%s: written outside the array" % k
        body = h[GUARD:-GUARD]
        out[k] = body if k in ("labels", "lens", "status") else body.reshape(B, T)
    return out


def assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k].astype(bool) if k == "masks" else got[k]
        if k == "masks":
            assert set(np.unique(got[k])) <= {0, 1}, (what, "masks holds bytes other than 0 / 1 (an element nobody wrote?)")
        assert g.shape == w.shape and np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5].tolist())


def batch_arrays(batch, with_ner):
    names = ("words", "masks") + tuple(k for k in OUT_IDS[1:] if with_ner or k != "ner")
    assert len(batch.inputs) == len(names)
    out = {k: t.cpu().numpy() for k, t in zip(names, batch.inputs)}
    for k in names:
        t = batch.inputs[names.index(k)]
        assert t.dtype == (torch.bool if k == "masks" else torch.int64) and t.is_contiguous()
    out.update(labels=batch.labels.cpu().numpy(), lens=batch.lens.cpu().numpy(), status=batch.status.cpu().numpy())
    assert batch.labels.dtype == torch.int64 and batch.lens.dtype == torch.int32 and batch.status.dtype == torch.int32
    return out


# (B, T) -> sentence numbers: repeats, the 45- and the 1-token sentence, indices outside the dataset
CASES = {
    (5, 45): [0, 1, 9, 9, 36],                                       # clean: T = Ts, the longest and the shortest sentence, a repeat
    (1, 45): [0],
    (33, 31): list(range(0, 30)) + [2, 3, 2],                        # odd T < Ts: sentences longer than 31 are empty rows
    (7, 64): [5, -1, 0, S, 1, 5, 36],                                # T > Ts, both kinds of bad index
    (4, 44): [4, 0, 1, 4],                                           # even T < Ts: the 45-token sentence does not fit
}


@pytest.mark.parametrize("with_ner", [True, False], ids=["tacred", "no_ner"])
@pytest.mark.parametrize("shape", sorted(CASES), ids=lambda s: "B%d_T%d" % s)
def test_assembly_is_bit_exact(dev, shape, with_ner):
    """Every output array of the launch, written into sentinel-filled buffers, against batch_ref; the same through DeviceDataset.batch;
    .check() raises for the first failing slot with its code and passes for the clean batches."""
    from gcn_over_pruned_trees_amd import dataset
    B, T = shape
    idx = CASES[shape]
    assert len(idx) == B
    ds, h = device_dataset(with_ner), host_view(with_ner)
    want = batch_ref.batch_ref(h, idx, T)
    assert_same(raw_gather(ds, idx, T), want, "C entry point")
    for given in (idx, torch.as_tensor(idx, dtype=torch.int64, device=dev)):
        batch = ds.batch(given, T)
        assert_same(batch_arrays(batch, with_ner), want, "DeviceDataset.batch")
    lens = host_dataset()["lens"]
    codes = [batch_ref.E_INVALID if (s < 0 or s >= S) else (batch_ref.E_LENGTH if lens[s] > T else 0) for s in idx]
    assert want["status"].tolist() == codes
    if shape == (33, 31):
        too_long = [b for b, s in enumerate(idx) if lens[s] > 31]
        assert len(too_long) >= 5 and 31 in lens[idx] and 32 in lens[idx]
        assert not want["lens"][too_long].any() and want["masks"][too_long].all() and (want["subj_pos"][too_long] == 150).all()
    if any(codes):
        first = next(b for b, c in enumerate(codes) if c)
        with pytest.raises(dataset.BatchError) as e:
            batch.check()
        assert (e.value.sentence, e.value.code) == (first, codes[first])
    else:
        assert batch.check() is batch
    if shape == (7, 64):
        assert codes.count(batch_ref.E_INVALID) == 2
        other = raw_gather(ds, idx, T, pos_fill=-5)
        assert (other["subj_pos"][want["masks"]] == -5).all() and np.array_equal(other["words"], want["words"])


def test_default_width_is_the_longest_sentence_of_the_batch(dev):
    ds, h = device_dataset(), host_dataset()
    for idx in ([2, 1, 7], [1], [0, 3], [1, -1, S + 4]):
        T = max([int(h["lens"][s]) for s in idx if 0 <= s < S])
        batch = ds.batch(np.asarray(idx))
        assert batch.T == T and tuple(batch.inputs[0].shape) == (len(idx), T)
        assert_same(batch_arrays(batch, True), batch_ref.batch_ref(h, idx, T), idx)
    with pytest.raises(ValueError, match="T is required"):
        ds.batch(torch.tensor([1, 2], device=dev))
    with pytest.raises(ValueError, match="int32"):
        from gcn_over_pruned_trees_amd import dataset
        big = h["words"].copy()
        big[0, 0] = 2 ** 31
        dataset.DeviceDataset.build(big, h["pos"], None, h["deprel"], h["head"], h["subj_pos"], h["obj_pos"], h["lens"], h["labels"], dev)


def test_word_dropout_follows_the_hash(dev):
    """Decisions bit-exact against the restated hash for two seeds and the device words 0 and 3; p = 0 is the plain copy; nothing but
    `words` depends on the seeds; a changed id is UNK_ID and was a real, non-UNK token; two slots with the same sentence differ; same seed
    same bits, another seed other bits.  Rate over all eligible tokens of the B = 37, T = 45 batch at p = 0.25 (threshold 16384 / 65536,
    exact): within 5 * sqrt(p (1 - p) / n) = 0.0746 of p for the n = 843 eligible tokens; observed 0.2598 / 0.2420 (seed 1234567, device
    word 0 / 3) and 0.2349 / 0.2562 (seed 2^40 + 99), the kernel's decisions being batch_ref's bit for bit."""
    ds, h = device_dataset(), host_dataset()
    idx, B, T, p = list(range(S)), S, TS, 0.25
    plain = raw_gather(ds, idx, T)
    assert_same(plain, batch_ref.batch_ref(h, idx, T), "p = 0")
    assert_same(raw_gather(ds, idx, T, p=0.0, seed=99), plain, "p = 0 ignores the seed")
    eligible = ~plain["masks"].astype(bool) & (plain["words"] != batch_ref.UNK_ID)
    n = int(eligible.sum())
    bound = 5.0 * np.sqrt(p * (1 - p) / n)
    seen = {}
    for seed in (1234567, 2 ** 40 + 99):
        for sd in (0, 3):
            got = raw_gather(ds, idx, T, p=p, seed=seed, seed_dev=torch.tensor([sd], dtype=torch.int64, device=dev))
            assert_same(got, batch_ref.batch_ref(h, idx, T, p=p, seed=seed, seed_dev=sd), (seed, sd))
            for k in plain:
                if k != "words":
                    assert np.array_equal(got[k], plain[k]), k
            changed = got["words"] != plain["words"]
            assert (got["words"][changed] == batch_ref.UNK_ID).all() and eligible[changed].all()
            rate = float(changed.sum()) / n
            print("word dropout seed %d seed_dev %d: %d of %d eligible tokens dropped, rate %.4f (bound +-%.4f)" % (seed, sd, changed.sum(), n, rate, bound))
            assert abs(rate - p) <= bound, (seed, sd, rate, n)
            seen[(seed, sd)] = got["words"]
        assert_same(raw_gather(ds, idx, T, p=p, seed=seed), dict(plain, words=seen[(seed, 0)]), "seed_dev NULL = 0")
        assert_same(raw_gather(ds, idx, T, p=p, seed=seed + 3), dict(plain, words=seen[(seed, 3)]), "seed and the device word add")
    assert len({v.tobytes() for v in seen.values()}) == 4
    # the key is the batch slot: the same sentence in two slots is dropped independently
    twice = raw_gather(ds, [0, 0, 0, 0], 45, p=p, seed=1234567)
    assert_same(twice, batch_ref.batch_ref(h, [0, 0, 0, 0], 45, p=p, seed=1234567), "repeated sentence")
    assert len({twice["words"][b].tobytes() for b in range(4)}) == 4
    # the Python surface: seed=None draws from the CPU generator, so torch.manual_seed fixes the batch
    torch.manual_seed(5)
    a = ds.batch(idx, T, word_dropout=p).inputs[0].cpu().numpy()
    c = ds.batch(idx, T, word_dropout=p).inputs[0].cpu().numpy()
    torch.manual_seed(5)
    b = ds.batch(idx, T, word_dropout=p).inputs[0].cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, plain["words"])
    assert np.array_equal(ds.batch(idx, T, word_dropout=p, seed=1234567).inputs[0].cpu().numpy(), seen[(1234567, 0)])


def small_model(gcn, dev, **kw):
    opt = dict(vocab_size=500, emb_dim=8, pos_dim=2, ner_dim=2, hidden_dim=24, num_layers=2, input_dropout=0.0, gcn_dropout=0.0, emb_dropout=0.0,
               word_dropout=0.0, prune_k=1, pooling="max", pooling_l2=0.003, mlp_layers=2, rnn=False, dataset="tacred", num_class=5, topn=1e10,
               cuda=True, adj_type="regular", gcn_check_trees=False, **kw)
    torch.manual_seed(77)
    return gcn.GCNClassifier(opt).to(dev)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.mark.parametrize("idx", [[0, 9, 9, 36, 20], [2, 12, 7]], ids=["five", "three"])
def test_model_on_a_device_batch_equals_the_host_path(api, dev, idx):
    """GCNClassifier on DeviceBatch.inputs with trees from the dataset's own TreeCache against the same model on tensors assembled on the
    host (batch_ref), uploaded, with trees pruned from them: the logits are bit-identical."""
    gcn, tree = api
    ds, h = device_dataset(), host_dataset()
    T = int(max(h["lens"][idx]))
    model = small_model(gcn, dev).eval()
    batch = ds.batch(idx)
    assert batch.T == T
    with torch.no_grad():
        got, _ = model(batch.inputs, trees=ds.tree_cache(1).batch(batch.idx, T))
        want_in = batch_ref.batch_ref(h, idx, T)
        host = tuple(to_dev(want_in[k], dev) for k in ("words", "masks", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos"))
        trees = tree.prune_to_csr(host[5], host[6], host[7], host[4], 1, masks=host[1], want_label=False)
        want, _ = model(host, trees=trees)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0 and _same_bits(got, want)


def test_captured_step_follows_the_index_buffer(api, dev):
    """The whole step -- batch gather, TreeCache.batch, forward, loss, backward, optimizer.step() -- as ONE hipGraph over a persistent idx
    tensor (B = 5, T = Ts, native head, native SGD, no word dropout).  After a copy of other sentence numbers into idx, a replay gives the
    loss and the logits of an eager step on those sentences from the same weights bit for bit, and the updated weights within the
    project's fp32 gradient bar, 1e-4 * max|reference|."""
    from gcn_over_pruned_trees_amd import optim
    gcn, _ = api
    ds = device_dataset()
    cache = ds.tree_cache(1, want_label=False)
    model = small_model(gcn, dev, gcn_native_head=True).train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = optim.get_optimizer("sgd", params, 0.3, 5.0)
    first, second = [0, 9, 20, 5, 36], [7, 4, 12, 12, 30]
    idx = torch.tensor(first, dtype=torch.int64, device=dev)
    second_dev = torch.tensor(second, dtype=torch.int64, device=dev)

    def step():
        batch = ds.batch(idx, TS)
        logits, pooled = model(batch.inputs, trees=cache.batch(idx, TS))
        loss = model.loss(logits, pooled, batch.labels)
        loss.backward()
        opt.step()
        return loss.detach(), logits.detach(), batch.inputs[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # warm-up: dense gradients exist (zeroed) from here on
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    start = [p.data.clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss, logits, words = step()

    def restart():
        for p, a in zip(params, start):
            p.data.copy_(a)
        opt.zero_grad()

    restart()
    idx.copy_(second_dev)
    graph.replay()
    torch.cuda.synchronize()
    got_loss, got_logits, got_words = loss.clone(), logits.clone(), words.clone()
    got = [p.data.clone() for p in params]
    restart()
    want_loss, want_logits, want_words = step()
    torch.cuda.synchronize()
    assert np.array_equal(got_words.cpu().numpy(), batch_ref.batch_ref(host_dataset(), second, TS)["words"])
    assert _same_bits(got_words, want_words) and _same_bits(got_loss, want_loss) and _same_bits(got_logits, want_logits)
    moved = 0
    for p, a, g in zip(params, start, got):
        ref = p.data
        scale = float(ref.abs().max())
        d = float((g - ref).abs().max())
        moved += float((ref - a).abs().max()) > 0
        print("captured step: param %s deviation %.3e, max|ref| %.3e" % (tuple(p.shape), d, scale))
        assert d <= GRAD_RTOL * scale, (tuple(p.shape), d, scale)
    assert moved >= 8
    # the first batch again through the same graph: it follows the buffer both ways
    restart()
    idx.copy_(torch.tensor(first, dtype=torch.int64, device=dev))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(words.cpu().numpy(), batch_ref.batch_ref(host_dataset(), first, TS)["words"]) and not _same_bits(loss, got_loss)


def test_captured_word_dropout_advances_with_the_device_word(dev):
    """A captured gather with word_dropout = 0.25 whose seed_dev counter is advanced by a captured add_: consecutive replays over the same
    idx give different words, each the restated hash's for the counter's value."""
    ds, h = device_dataset(), host_dataset()
    first = [0, 9, 20, 5, 36]
    idx = torch.tensor(first, dtype=torch.int64, device=dev)
    counter = torch.zeros((1,), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ds.batch(idx, TS, word_dropout=0.25, seed=42, seed_dev=counter)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        counter.add_(1)
        batch = ds.batch(idx, TS, word_dropout=0.25, seed=42, seed_dev=counter)
    seen = []
    for replay in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(counter) == replay
        seen.append(batch.inputs[0].cpu().numpy().copy())
        assert np.array_equal(seen[-1], batch_ref.batch_ref(h, first, TS, p=0.25, seed=42, seed_dev=replay)["words"])
        assert np.array_equal(batch.inputs[6].cpu().numpy(), batch_ref.batch_ref(h, first, TS)["subj_pos"])
    assert len({w.tobytes() for w in seen}) == 3
