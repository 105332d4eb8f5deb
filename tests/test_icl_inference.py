"""`icl_inference` / `random_ice_idx_list` of the inference mirror (ref:inference.py:206-211, 323-377) with the fake processor and
stub model of tests/test_inference_tail.py: prompt layout, demonstration order, chunking, the bs-wide last chunk, result records."""
import random
import types

import torch

import inference as I
from test_inference_tail import FakeTokenizer, StubModel


def _setup(n_val=5, bs=2):
    seen = []

    def prepare_input(prompts):
        seen.append([list(p) for p in prompts])
        n = len(prompts)
        return dict(input_ids=torch.full((n, 3), 4), attention_mask=torch.ones(n, 3, dtype=torch.long))

    proc = types.SimpleNamespace(tokenizer=FakeTokenizer(), prepare_input=prepare_input)
    pm = types.SimpleNamespace(
        gen_query_text_without_label=lambda s: f"Question:{s['question']} Short answer:",
        gen_ice_text_with_label=lambda s, add_sep_token=False: f"Question:{s['question']} Short answer:{s['answer']}" + ("<sep>" if add_sep_token else ""))
    train = [dict(image=f"timg{i}", question=f"tq{i}", answer=f"a{i}") for i in range(10)]
    val = [dict(image=f"img{i}", question=f"q{i}", question_id=100 + i) for i in range(n_val)]
    model = StubModel(torch.tensor([[20 + i, 2] for i in range(bs)]))
    return seen, proc, pm, train, val, model


def test_prompts_hold_the_demonstrations_in_list_order_then_the_query():
    seen, proc, pm, train, val, model = _setup()
    ice = [[3, 1], [7, 0], [2, 2], [9, 8], [5, 4]]
    res = I.icl_inference(train, val, ice, model, pm, proc, bs=2, generate_kwargs=dict(num_beams=3), instruction="Answer briefly.")
    assert seen[0][0] == ["Answer briefly.", "timg3", "Question:tq3 Short answer:a3<sep>", "timg1", "Question:tq1 Short answer:a1<sep>",
                          "img0", "Question:q0 Short answer:"]
    assert seen[1][1][1:5] == ["timg9", "Question:tq9 Short answer:a9<sep>", "timg8", "Question:tq8 Short answer:a8<sep>"]
    assert [len(p) for p in seen] == [2, 2, 2]                                   # last chunk still bs prompts wide
    assert seen[2][1] == ["Answer briefly."] and seen[2][0][-2:] == ["img4", "Question:q4 Short answer:"]
    assert list(res) == [0, 1, 2, 3, 4]
    assert res[3] == {"prediction": "t21", "question": "q3", "question_id": 103}
    assert "image" in val[0] and "image" in train[3]                             # nobody's samples are mutated
    assert all(c["icv"] is None and c["num_beams"] == 3 for c in model.calls) and len(model.calls) == 3


def test_without_instruction_and_with_zero_shots():
    seen, proc, pm, train, val, model = _setup(n_val=2)
    res = I.icl_inference(train, val, [[], [6]], model, pm, proc, bs=2, generate_kwargs={})
    assert seen[0][0] == ["img0", "Question:q0 Short answer:"]
    assert seen[0][1] == ["timg6", "Question:tq6 Short answer:a6<sep>", "img1", "Question:q1 Short answer:"]
    assert [r["prediction"] for r in res.values()] == ["t20", "t21"]


def test_random_ice_idx_list_draws_distinct_indices_as_the_reference_does():
    got = I.random_ice_idx_list(50, 7, 4, random.Random(5))
    rng, pool = random.Random(5), list(range(50))
    assert got == [rng.sample(pool, 4) for _ in range(7)]                        # ref:inference.py:206-211 with the same generator
    assert all(len(set(r)) == 4 and all(0 <= v < 50 for v in r) for r in got) and len(got) == 7
    random.seed(9)
    a = I.random_ice_idx_list(20, 3, 2)
    random.seed(9)
    assert a == I.random_ice_idx_list(20, 3, 2)                                  # default: the module-level generator


def test_prompt_manager_of_the_package_formats_a_demonstration():
    from lmm_icl_interface.prompt import LMMPromptManager  # noqa: F401  (the real class has the method icl_inference calls)
    assert hasattr(LMMPromptManager, "gen_ice_text_with_label") and hasattr(LMMPromptManager, "gen_query_text_without_label")
