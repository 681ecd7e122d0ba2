"""CPU: tests/head_cases.py draws the bytes that tests/golden/head_cases.json records.  The file was
recorded from the functions head_cases.py replaced (its first key says how), so these tests are the
proof that moving the add-on suites onto one module changed no input byte, and they keep a later edit
of a draw from going unnoticed.  The helpers that make assertions for the GPU suites are exercised
on the host as well: a check that cannot fail checks nothing."""
import hashlib
import json
import os

import pytest
import torch

from tests import head_cases as HC

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_cases.json")))
GRID_STRIDE = ((2, (1, 513, 1023)), (2, (1, 200, 300)), (2, (1, 257, 511)))


def digest(t):
    t = t.contiguous()
    h = hashlib.sha256(f"{t.dtype} {tuple(t.shape)} ".encode())
    h.update(t.numpy().tobytes())
    return h.hexdigest()


def test_head_inputs_are_the_recorded_bytes():
    cases = [(nc, shape) for nc in HC.CLASSES for shape in HC.SHAPES] + list(GRID_STRIDE)
    assert sorted(GOLDEN["head_inputs"]) == sorted(f"{nc} {s[0]}x{s[1]}x{s[2]}" for nc, s in cases)
    for nc, shape in cases:
        x, w, b = HC.head_inputs(nc, shape)
        assert tuple(x.shape) == (shape[0], 16) + shape[1:]
        assert tuple(w.shape) == (16, nc, 2, 2) and tuple(b.shape) == (nc,)
        want = GOLDEN["head_inputs"][f"{nc} {shape[0]}x{shape[1]}x{shape[2]}"]
        assert {"x": digest(x), "w": digest(w), "b": digest(b)} == want, (nc, shape)
        assert HC.head_inputs(nc, shape)[0] is x                # cached: one draw for every suite


def test_targets_and_look_up_tables_are_the_recorded_bytes():
    assert len(GOLDEN["make_target"]) == 8
    for entry in GOLDEN["make_target"]:
        nc, shape, ignore, seed = entry["args"]
        assert digest(HC.make_target(nc, tuple(shape), ignore, seed)) == entry["sha256"], entry["args"]
    for nc in HC.CLASSES:
        ids, pal = HC.random_luts(nc)
        assert {"id_map": digest(ids), "palette": digest(pal)} == GOLDEN["random_luts"][str(nc)], nc
        assert digest(HC.random_palette(nc)) == GOLDEN["random_palette"][str(nc)], nc


def test_the_arena_is_the_layout_the_suites_used_and_sees_a_stray_byte():
    sizes = {"a": 1, "b": 3 * 77, "c": 4 * 77}
    arena = HC.Arena(torch.device("cpu"), sizes)
    off_a = 256
    off_b = (off_a + 1 + 256 + 15) // 16 * 16
    off_c = (off_b + 3 * 77 + 256 + 15) // 16 * 16
    assert arena.off == {"a": off_a, "b": off_b, "c": off_c}
    assert arena.buf.numel() == (off_c + 4 * 77 + 256 + 15) // 16 * 16 and (arena.buf == 0xA5).all()
    assert [arena.ptr(k) - arena.buf.data_ptr() for k in sizes] == [off_a, off_b, off_c]
    arena.buf[off_b:off_b + 3 * 77] = 1
    arena.read()
    assert (arena.cut("b") == 1).all() and arena.cut("b").numel() == 3 * 77
    arena.assert_untouched(("b",))
    with pytest.raises(AssertionError):
        arena.assert_untouched(())                              # "b" was written and not named
    for stray in (0, off_a + 1, off_b - 1, off_b + 3 * 77, arena.buf.numel() - 1):
        arena.buf.fill_(0xA5)
        arena.buf[stray] = 0
        arena.read()
        with pytest.raises(AssertionError):
            arena.assert_untouched(("a", "b", "c") if stray != off_a + 1 else ("b", "c"))


def test_check_labels_and_its_two_policies():
    ref = torch.arange(2000).reshape(1, 40, 50) % 7
    label = ref.to(torch.uint8)
    none = torch.zeros_like(ref, dtype=torch.bool)
    two, three = none.clone(), none.clone()
    two.view(-1)[:2] = True
    three.view(-1)[:3] = True
    assert [HC.cap(n) for n in (1, 99, 100, 1999, 2000, 2999, 3000)] == [0, 0, 1, 1, 2, 2, 3]
    for limit in (HC.share(1e-3), HC.count_cap):
        HC.check_labels(label, ref, none, "clean", limit)
        HC.check_labels(label, ref, two, "two of 2000", limit)
        with pytest.raises(AssertionError, match="near-ties"):
            HC.check_labels(label, ref, three, "three of 2000", limit)
        wrong = label.clone()
        wrong[0, 0, 1] += 1
        HC.check_labels(wrong, ref, two, "wrong where excluded", limit)
        wrong[0, 0, 5] += 1
        with pytest.raises(AssertionError, match="1 of 2000 labels differ"):
            HC.check_labels(wrong, ref, two, "wrong outside", limit)
        with pytest.raises(AssertionError):
            HC.check_labels(label.long(), ref, none, "not u8", limit)
    with pytest.raises(AssertionError, match="near-ties"):
        HC.count_cap(torch.ones(99, dtype=torch.bool), "fewer than 100 pixels")


def test_near_tie_is_the_two_gamma_s_rule():
    """A margin of 3e-6 between classes 0 and 1, whose larger S is 2: the bound 4 gamma_k reaches it from k = 13 on."""
    logits = torch.tensor([1.0, 1.0 - 3e-6, 0.0], dtype=torch.float64).reshape(1, 3, 1, 1)
    S = torch.tensor([1.0, 2.0, 9.0], dtype=torch.float64).reshape(1, 3, 1, 1)
    assert HC.gamma(17) == 17 * HC.U / (1 - 17 * HC.U) and 4 * HC.gamma(12) < 3e-6 < 4 * HC.gamma(13)
    assert HC.near_tie(logits, S, 13).item() and not HC.near_tie(logits, S, 12).item()
