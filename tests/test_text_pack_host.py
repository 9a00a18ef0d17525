"""CPU: the packing plan of the text tower (which rows a batch of captions needs) restated in torch, and the engine's decision
when to pack.

`plan_ref` is the reference of the GPU plan test (tests/test_hip_text_pack.py): len[b] = argmax(ids[b]) + 1 with the first
maximum winning, start = exclusive sum in batch order, last_row = start + len - 1, totals = (rows, longest caption).  It is
written with plain Python loops so that it shares nothing with the engine's own torch form (engine.text_pack_plan_host),
which is checked against it here.
"""
import pytest
import torch


def plan_ref(ids):
    """(len [B], start [B+1], last_row [B], (rows, max_len)) as Python lists, from an int64 [B, L] id tensor."""
    lens, start, last = [], [0], []
    for row in ids.tolist():
        best, at = row[0], 0
        for t, v in enumerate(row):
            if v > best:                      # strictly greater: the first maximum wins
                best, at = v, t
        lens.append(at + 1)
        last.append(start[-1] + at)
        start.append(start[-1] + at + 1)
    return lens, start, last, (start[-1], max(lens))


EOT = 49407
HAND = {
    "eot_first": (torch.tensor([[EOT, 5, 6, 7, 0, 0]]), [1], [0, 1], [0], (1, 1)),
    "eot_last": (torch.tensor([[3, 5, 6, 7, 9, EOT]]), [6], [0, 6], [5], (6, 6)),
    "two_maxima": (torch.tensor([[1, EOT, 4, EOT, 0, 0]]), [2], [0, 2], [1], (2, 2)),
    "all_zero": (torch.tensor([[0, 0, 0, 0, 0, 0]]), [1], [0, 1], [0], (1, 1)),
    "mixed": (torch.tensor([[EOT, 5, 6, 7, 0, 0], [3, 5, 6, 7, 9, EOT], [1, EOT, 4, EOT, 0, 0], [0, 0, 0, 0, 0, 0],
                            [2, 9, EOT, 0, 0, 0]]),
              [1, 6, 2, 1, 3], [0, 1, 7, 9, 10, 13], [0, 6, 8, 9, 12], (13, 6)),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_plan_on_hand_made_ids(name):
    """EOT at position 0 (len 1), at the last position (len = L), two equal maxima (the first wins), an all-zero row, B = 1 and
    a batch of all of them: the restatement gives the hand-computed plan, torch.argmax agrees, and so does the engine's form."""
    from vitlens_hip import engine
    ids, lens, start, last, total = HAND[name]
    assert plan_ref(ids) == (lens, start, last, total)
    assert (ids.argmax(dim=-1) + 1).tolist() == lens
    l, s, r, t = engine.text_pack_plan_host(ids)
    assert l.dtype == torch.int32 and s.dtype == torch.int32 and r.dtype == torch.int64
    assert (l.tolist(), s.tolist(), r.tolist(), t) == (lens, start, last, total)


def test_plan_on_random_ids_matches_argmax():
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 50, (37, 77), generator=g)          # few distinct values: many ties
    lens, start, last, (rows, mx) = plan_ref(ids)
    assert lens == (ids.argmax(dim=-1) + 1).tolist()
    assert rows == sum(lens) and mx == max(lens) and last == [s + n - 1 for s, n in zip(start, lens)]


def test_pack_mode(monkeypatch):
    """The decision function: packed only for the fp16 arithmetic on a GPU with the switch on; "host" for CPU tokens, "device"
    for GPU tokens; dense while the current stream is being captured into a graph."""
    from vitlens_hip import engine
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    cpu_ids = torch.zeros(2, 77, dtype=torch.long)

    class _Dev:                  # stands in for a token tensor on the GPU
        is_cuda = True
    assert engine.text_pack_mode("f16", cpu_ids, "cuda:0") == "host"
    assert engine.text_pack_mode("f16", _Dev(), "cuda:0") == "device"
    for arith in ("bf16x2", "bf16"):
        assert engine.text_pack_mode(arith, _Dev(), "cuda:0") == "dense"
    assert engine.text_pack_mode("f16", cpu_ids, "cpu") == "dense"
    monkeypatch.setattr(engine, "PACK_TEXT", False)
    assert engine.text_pack_mode("f16", _Dev(), "cuda:0") == "dense"
    monkeypatch.setattr(engine, "PACK_TEXT", True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert engine.text_pack_mode("f16", _Dev(), "cuda:0") == "dense"
    assert engine.text_pack_mode("f16", cpu_ids, "cuda:0") == "dense"


def test_capturing_stream_requests_no_plan(monkeypatch):
    """Under a capture plan_text returns None - the dense path - without launching the plan kernel or reading anything back
    (no graph is captured here: the decision is what is tested)."""
    from vitlens_hip import engine
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    eng = object.__new__(engine.TextEngine)
    eng.arith, eng.device = "f16", torch.device("cuda:0")

    def boom(*a, **k):
        raise AssertionError("a capture must not request a device read")
    monkeypatch.setattr(engine.TextEngine, "_plan_on_device", boom)
    monkeypatch.setattr(engine, "text_pack_plan_host", boom)

    class _Dev:
        is_cuda = True
        shape = (4, 77)
    assert eng.plan_text(_Dev()) is None
    assert eng.plan_text(torch.zeros(4, 77, dtype=torch.long)) is None
    # and outside a capture the device form IS what a GPU token tensor asks for
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    with pytest.raises(AssertionError, match="device read"):
        eng.plan_text(_Dev())


def test_steps_ask_for_the_plan_only_where_the_engine_has_one():
    """A frozen-text stand-in without plan_text (tests/test_step_gloo.py's stubs, a CPU device) keeps working."""
    from vitlens_hip import step

    class _Stub:
        def encode_text(self, t):
            return t
    st = object.__new__(step._StepState)
    st.text = _Stub()
    texts = torch.zeros(2, 77, dtype=torch.long)
    assert st._text_plan(texts) is None
    assert st._encode_text(texts, None) is texts


def test_step_classes_choose_whether_to_pack():
    """A step class with `pack_text` off (the point-cloud step: its host-bound front pays for the plan's host wait) asks for
    no plan and tells the engine to run dense; the others ask at any batch size and hand the plan on."""
    from vitlens_hip import step
    calls = []

    class _Eng:
        def plan_text(self, t):
            calls.append("plan")
            return "PLAN"

        def encode_text(self, t, plan=None):
            calls.append(("encode", plan))
            return t
    assert step.TriModalDepthStep.pack_text and step.DualAudioStep.pack_text and not step.TriModalPCStep.pack_text
    texts = torch.zeros(2, 77, dtype=torch.long)
    st = object.__new__(step.TriModalPCStep)
    st.text = _Eng()
    assert st._text_plan(texts) is None and calls == []
    st._encode_text(texts, None)
    assert calls == [("encode", False)]
    del calls[:]
    for cls in (step.TriModalDepthStep, step.DualAudioStep):
        st = object.__new__(cls)
        st.text = _Eng()
        st._encode_text(texts, st._text_plan(texts))
    assert calls == ["plan", ("encode", "PLAN")] * 2
