"""The conditions the inputs of the batched verification tests (tests/verify_batched_cases.py) must meet, checked on the
numpy rule alone (no GPU), so that the mistakes a batched kernel can make show in tests/test_gpu_verify_batched.py:

* no two pairs of a batch that have a winner share their model or their mask -- a pair mix-up or a wrong row offset
  shows (the short and the empty pairs all have the zero model: they are told apart by their `matches` field);
* the (120, 80) and (300, 300) pairs sit at p > 0 and their reference with seed + p differs from the one with the
  call's seed -- a kernel that ignores p in the seed shows; MIXED's seed wraps past 2^32 inside the batch;
* the short pairs and the empty pair give hypothesis = -1;
* CAPPED's tail changes the result when it is counted, so the device counter matters;
* sift_amd.multi.position_pairs agrees with code_pairs' order and counts for world 1, 2 and 8, on CPU tensors.
"""
import numpy as np
import pytest

import verify_batched_cases as bc


@pytest.mark.parametrize("model", bc.MODELS)
@pytest.mark.parametrize("batch", ["MIXED", "LARGE64", "FULL"])
def test_no_two_pairs_share_a_model_or_a_mask(model, batch):
    P = len(bc.pairs(model, batch))
    refs = [bc.reference(model, batch, p) for p in range(P)]
    won = [p for p in range(P) if refs[p]["hypothesis"] >= 0]
    assert len(won) == {"MIXED": 5, "LARGE64": 2, "FULL": 64}[batch]
    models = {bc.model_of(model, refs[p]).tobytes() for p in won}
    masks = {refs[p]["mask"].tobytes() for p in won}
    lists = {refs[p]["list"].tobytes() for p in won}
    assert len(models) == len(masks) == len(lists) == len(won)
    for p in won:
        assert refs[p]["inliers"] >= bc.SAMPLE[model] and refs[p]["matches"] == bc.pairs(model, batch)[p]["count"]


def test_batch_shapes():
    for model in bc.MODELS:
        caps = bc.caps(model, "MIXED")
        assert caps == [sum(bc.SHORT[model]), 200, 0, 200, 600, 33, 2113]
        assert all(c % 64 for c in caps if c) and len(bc.matches(model, "MIXED")) == sum(caps)
        assert bc.counts(model, "MIXED").tolist() == [caps[0], 200, 0, 129, 600, 33, 2113]
        assert max(caps) > 2048 and bc.row0(model, "MIXED")[-2] % 64  # the large pair starts at an odd row
        assert bc.caps(model, "FULL") == [33] * 64
        K, seed = bc.BATCHES["MIXED"]
        assert K == 256 and seed + 2 < bc.U32 <= seed + 3  # the seed wraps inside the batch
    assert sum(bc.SPILL["caps"]) <= bc.SPILL["max_matches"] and max(bc.SPILL["caps"]) > 65536 >= min(bc.SPILL["caps"])


@pytest.mark.parametrize("model", bc.MODELS)
def test_the_pair_index_shows_in_the_seed(model):
    shapes = [p["shape"] for p in bc.pairs(model, "MIXED")]
    for shape in ((120, 80), (300, 300)):
        p = shapes.index(shape)
        assert p > 0
        with_p, without = bc.reference(model, "MIXED", p), bc.reference(model, "MIXED", p, seed_offset=False)
        assert not np.array_equal(with_p["samples"], without["samples"])
        assert with_p["hypothesis"] != without["hypothesis"] or \
            bc.model_of(model, with_p).tobytes() != bc.model_of(model, without).tobytes()
    for p in range(1, 64):  # FULL: every pair's draw differs from the one its own list would get at p = 0
        assert not np.array_equal(bc.reference(model, "FULL", p)["samples"],
                                  bc.reference(model, "FULL", p, seed_offset=False)["samples"])


@pytest.mark.parametrize("model", bc.MODELS)
def test_short_and_empty_pairs_have_no_winner(model):
    shapes = [p["shape"] for p in bc.pairs(model, "MIXED")]
    for shape in (bc.SHORT[model], "empty"):
        p = shapes.index(shape)
        for counted in (True, False):
            r = bc.reference(model, "MIXED", p, counted)
            assert r["hypothesis"] == -1 and r["inliers"] == 0 and r["valid_hypotheses"] == 0
            assert not bc.model_of(model, r).any() and not r["mask"].any() and len(r["list"]) == 0
            assert r["matches"] == (0 if shape == "empty" else sum(shape))


@pytest.mark.parametrize("model", bc.MODELS)
def test_the_capped_tail_changes_the_result(model):
    p = [q["shape"] for q in bc.pairs(model, "MIXED")].index("capped")
    head, whole = bc.reference(model, "MIXED", p, True), bc.reference(model, "MIXED", p, False)
    assert (head["matches"], whole["matches"]) == (129, 200)
    assert not np.array_equal(head["samples"], whole["samples"])
    assert bc.model_of(model, head).tobytes() != bc.model_of(model, whole).tobytes()


@pytest.mark.parametrize("world", [1, 2, 8])
def test_position_pairs_follow_code_pairs(world):
    import torch

    from sift_amd import multi

    n, c = 40, 3
    gathered = torch.arange(world * n * c, dtype=torch.float32).reshape(world, n, c)
    counts = [n - 3 * r for r in range(world)]
    n_pad = multi.code_block_rows(n)
    for rank in range(world):
        got = multi.position_pairs(gathered, counts, rank, world)
        codes = multi.code_pairs(counts, rank, world, n_pad)
        peers = multi.peer_pairs(rank, world)
        assert len(got) == len(codes) == len(peers) == world - 1
        for (q_ptr, nq, t_ptr, nt), code, (_, j) in zip(got, codes, peers):
            assert (nq, nt) == (code[2], code[5]) == (counts[rank], counts[j])
            assert q_ptr == gathered[rank].data_ptr() == gathered.data_ptr() + 4 * rank * n * c
            assert t_ptr == gathered[j].data_ptr() == gathered.data_ptr() + 4 * j * n * c
    with pytest.raises(ValueError):
        multi.position_pairs(gathered.double(), counts, 0, world)
    with pytest.raises(ValueError):
        multi.position_pairs(gathered[:, :, :2], counts, 0, world)  # not rows of c floats any more
    with pytest.raises(ValueError):
        multi.position_pairs(gathered, counts, 0, world + 1)
