"""tools/beam_group_bench.py without a GPU: the diversity statistics by hand, the result line's ratios, and the statistics on a host-law
search where the answer is known (a penalty above the logits' spread makes the groups open with pairwise different words)."""
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from valor_amd import decode  # noqa: E402
import test_beam_pool_cpu as C  # noqa: E402

_spec = importlib.util.spec_from_file_location("beam_group_bench", os.path.join(ROOT, "tools", "beam_group_bench.py"))
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)                                          # (its main() is what needs the device; importing it does not)

SEP = 2


def test_diversity_statistics_by_hand():
    # clip 0: [5 6 7], [5 6 7] (a duplicate), [5 6 8]: 2 distinct; bigrams (5,6) (6,7) (5,6) (6,7) (5,6) (6,8): 3 distinct of 6
    # clip 1: [9], [SEP ...] (empty), [4 4 4 4] (no [SEP]): 3 distinct; bigrams (4,4) x 3: 1 distinct of 3
    seqs = [[5, 6, 7, SEP], [5, 6, 7, SEP], [5, 6, 8, SEP], [9, SEP, 3, 3], [SEP, SEP, SEP, SEP], [4, 4, 4, 4]]
    assert bench.diversity(seqs, 3, SEP) == (2.5, round((3 / 6 + 1 / 3) / 2, 4))
    assert bench.diversity(torch.tensor(seqs), 3, SEP) == bench.diversity(seqs, 3, SEP)
    assert bench.diversity([[SEP, SEP], [7, SEP]], 2, SEP) == (2.0, 0.0)              # no bigram at all
    assert bench.diversity(seqs, 1, SEP)[0] == 1.0


def test_result_line():
    runs = {(4, 1): [0.5, 0.5], (4, 2): [0.625, 0.625], (8, 2): [1.0, 1.0]}
    burst = {c: {"vocab": [20.0 * c[1], 20.0 * c[1]], "vocab64": [5.0, 7.0]} for c in runs}
    res = bench.summarise({"batch": 64}, 64, runs, burst, {c: (3.5, 0.75) for c in runs})
    assert res["pool_beam4"]["captions_per_s"] == [128.0, 128.0] and "captions_per_s_vs_pool" not in res["pool_beam4"]
    g = res["group_beam4_groups2"]
    assert g["captions_per_s_vs_pool"] == 0.8 and g["step_launch_vs_pool"] == 2.0 and g["step_launch_vs_pool_vocab64"] == 1.0
    assert g["distinct_sequences_of_n"] == 3.5 and g["distinct_bigram_share"] == 0.75 and g["n"] == 4
    assert "captions_per_s_vs_pool" not in res["group_beam8_groups2"]                 # no pool search of beam 8 in this run
    assert bench.name(8, 1) == "pool_beam8" and set(bench.CONFIGS) == {(4, 1), (8, 1), (4, 2), (4, 4), (8, 2), (8, 4)}


def test_statistics_on_a_host_law_search():
    """every slot reads the same row (a decoder's rows depend on the words alone at step 0) and the penalty 16 exceeds the spread of the
    quantised logits (4.5 + the [SEP] offset): at step 0 no group takes a word an earlier group took, and a group's hypotheses descend
    from its own step-0 words, so the n = K returned are pairwise distinct and the first G open with G different words"""
    b, K, G, L_, V_ = 2, 4, 2, 7, 20
    script = [z[:b].repeat(K, 1) for z in C.random_script(5, b, K, L_, V_, SEP)]
    script[0][:, SEP] = -float("inf")                                    # ([SEP] is never penalised: both groups could open with it)
    seqs, _, _, _, group = decode.decode_beam_pool_host(script, b, K, L_, None, None, K, eos=SEP, num_beam_groups=G, diversity_penalty=16.0)
    distinct, share = bench.diversity(seqs.reshape(b * K, L_), K, SEP)
    assert distinct == float(K) and 0.0 < share <= 1.0
    for s in range(b):
        first = {int(group[s, j]): int(seqs[s, j, 0]) for j in range(G)}
        assert len(first) == G and len(set(first.values())) == G
