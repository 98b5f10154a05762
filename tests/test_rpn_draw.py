"""The RPN sampler's draws as data: mt19937.MT.sampler_draws (numpy: RandomSampler's decisions and its
torch.randperm(n)[:k] draws on torch's CPU engine, the statement a device-side draw has to meet) against
rpn_train.sample_plan on the same seeded torch.Generator -- ranks, sampled counts, `all` flags and the generator
afterwards, bit for bit."""
import numpy as np
import pytest
import torch

from attentionshift_amd import mt19937 as M, rpn_train as RT

PERM_LIMIT = 0xFFFFFFFF // 20                     # torch.randperm's simple loop ends here

# name -> (counts per image, num, k_pos, neg_pos_ub, words consumed from a fresh seed before the call)
CASES = {
    "smallest": ([(3, 5)], 4, 2, -1, 0),                                   # both sets draw; a fresh seed has left == 1
    "all-fit": ([(2, 2)], 256, 128, -1, 10),
    "empty": ([(0, 0)], 256, 128, -1, 10),
    "one-more-then-exact": ([(129, 129), (128, 128)], 256, 128, -1, 10),
    "pos-then-neg": ([(200, 50), (10, 5000)], 256, 128, -1, 10),
    "no-pos-no-neg": ([(0, 900), (700, 0)], 256, 128, -1, 10),
    "shipped": ([(38, 261546), (8, 261386), (300, 259000)], 256, 128, -1, 10),
    "cap": ([(2049, 2049), (5000, 3000)], 2048, 1024, -1, 10),
    "full-table": ([(0, 300000)], 2048, 1024, -1, 10),                     # 2048 swaps, nearly all with a far end past k
    "bounded-3": ([(0, 500), (5, 500)], 64, 32, 3, 10),
    "bounded-half": ([(0, 500), (5, 500)], 64, 32, 0.5, 10),
}
# refill seams: the first draw finds `left` at these values.  A fresh seed has left == 1; its first word refills and leaves
# 624, so c >= 1 consumed words leave 625 - c.  The positives' 128-draw chain then crosses a block boundary (left 1, 2, 128)
# or ends on it (left 129: exactly 128 words remain)
SEAM_LEFTS = (1, 2, 128, 129, 624)
for _left in SEAM_LEFTS:
    CASES[f"seam-left{_left}"] = ([(129, 700), (129, 700)], 256, 128, -1, 0 if _left == 1 else 625 - _left)


def generator_at(consumed, seed=1234):
    """a CPU generator `consumed` engine words after its seed"""
    gen = torch.Generator().manual_seed(seed)
    if consumed:
        torch.randint(1 << 20, (consumed,), generator=gen)                 # one word per element
    return gen


def host_plan(counts, num, k_pos, neg_pos_ub, gen):
    """rpn_train.sample_plan in sampler_draws' output format (pos_fraction = k_pos / num is exact for the cases here)"""
    assert int(num * (k_pos / num)) == k_pos
    plan = np.zeros((len(counts), 4), dtype=np.int32)
    ranks = np.zeros((len(counts), 2, num), dtype=np.int32)
    for b, (pos_r, n_ps, neg_r, n_ns) in enumerate(RT.sample_plan(counts, num, k_pos / num, neg_pos_ub, gen)):
        plan[b] = (n_ps, pos_r is None, n_ns, neg_r is None)
        if pos_r is not None:
            ranks[b, 0, :n_ps] = pos_r.numpy()
        if neg_r is not None:
            ranks[b, 1, :n_ns] = neg_r.numpy()
    return plan, ranks


@pytest.mark.parametrize("name", list(CASES))
def test_sampler_draws_equal_sample_plan_and_leave_the_generator_alike(name):
    counts, num, k_pos, ub, consumed = CASES[name]
    gen = generator_at(consumed)
    blob = gen.get_state()
    mt = M.MT(M.unpack_state(blob))
    if name.startswith("seam-left"):
        assert mt.left == int(name[len("seam-left"):])
    plan, ranks, flag = mt.sampler_draws(counts, num, k_pos, ub)
    want_plan, want_ranks = host_plan(counts, num, k_pos, ub, gen)
    assert flag == 0
    assert np.array_equal(plan, want_plan), (plan, want_plan)
    assert np.array_equal(ranks, want_ranks)
    assert torch.equal(M.pack_state(blob, mt.compact()), gen.get_state())
    drew = bool((plan[:, 1] == 0).any() or (plan[:, 3] == 0).any())
    assert drew != torch.equal(blob, gen.get_state())                      # a set that fits consumes nothing


def test_the_cases_cover_what_they_are_named_for():
    plan = {k: M.MT(M.unpack_state(generator_at(c[4]).get_state())).sampler_draws(*c[:4])[0].tolist() for k, c in CASES.items()}
    assert plan["smallest"] == [[2, 0, 2, 0]]
    assert plan["all-fit"] == [[2, 1, 2, 1]] and plan["empty"] == [[0, 1, 0, 1]]
    assert plan["one-more-then-exact"] == [[128, 0, 128, 0], [128, 1, 128, 1]]
    assert plan["pos-then-neg"] == [[128, 0, 50, 1], [10, 1, 246, 0]]
    assert plan["no-pos-no-neg"] == [[0, 1, 256, 0], [128, 0, 0, 1]]
    assert plan["shipped"] == [[38, 1, 218, 0], [8, 1, 248, 0], [128, 0, 128, 0]]
    assert plan["cap"] == [[1024, 0, 1024, 0], [1024, 0, 1024, 0]]
    assert plan["full-table"] == [[0, 1, 2048, 0]]
    assert plan["bounded-3"] == [[0, 1, 3, 0], [5, 1, 15, 0]]              # int(3 * max(1, 0)), int(3 * 5)
    assert plan["bounded-half"] == [[0, 1, 0, 0], [5, 1, 2, 0]]            # int(0.5 * 1) = 0 draws nothing but skips 499 words
    lefts = sorted(M.MT(M.unpack_state(generator_at(CASES[f"seam-left{v}"][4]).get_state())).left for v in SEAM_LEFTS)
    assert lefts == sorted(SEAM_LEFTS)


@pytest.mark.parametrize("n,k", [(300, 128), (129, 128), (625, 256), (5000, 2048), (261546, 218)])
def test_randperm_first_reproduces_torch(n, k):
    gen = generator_at(10)
    blob = gen.get_state()
    mt = M.MT(M.unpack_state(blob))
    assert mt.randperm_first(n, k) == torch.randperm(n, generator=gen)[:k].tolist()
    assert torch.equal(M.pack_state(blob, mt.compact()), gen.get_state())


def test_flagged_counts_consume_nothing_and_the_other_images_still_draw():
    for bad in ((-1, 500), (500, -1), (PERM_LIMIT, 500), (500, PERM_LIMIT)):
        gen = generator_at(10)
        blob = gen.get_state()
        mt = M.MT(M.unpack_state(blob))
        plan, ranks, flag = mt.sampler_draws([(200, 300), bad, (10, 400)], 64, 32, -1)
        want_plan, want_ranks = host_plan([(200, 300), (10, 400)], 64, 32, -1, gen)
        assert flag == 1 and plan[1].tolist() == [0, 0, 0, 0] and not ranks[1].any()
        assert np.array_equal(plan[[0, 2]], want_plan) and np.array_equal(ranks[[0, 2]], want_ranks)
        assert torch.equal(M.pack_state(blob, mt.compact()), gen.get_state())
    with pytest.raises(ValueError):
        M.MT(M.unpack_state(generator_at(10).get_state())).sampler_draws([(1, 1)], 64, 65, -1)
