"""Memo rows: which cos / exp of a feature gets which register row of the eval chain — the host-only choice
(`de_memo_rows_assign`, csrc/de_bind.h memo_assign), the function a program calls on its tightest assured tier.  No GPU.

A candidate is an instruction of the ASSURED stream whose id is the untested cos / exp of a row (TOPA_UNROW_BASE + k * 8 + push * 2)
and whose operand row is a feature; the n_rows most frequent (operator, feature) pairs get a row, ties to the smaller pair."""
from collections import Counter

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api
import test_assured as ta

OPS = de.synth.BENCH_OPERATORS
COS, EXP = OPS.unaops.index("cos") + 1, OPS.unaops.index("exp") + 1
ADD, MUL = OPS.binops.index("+") + 1, OPS.binops.index("*") + 1
PLAIN = {ta.TOPA["UNROW"] + k * 8 + push * 2: k for k in (0, 1) for push in (0, 1)}  # id -> operator (0 cos, 1 exp)


def X(f):
    return de.Node(feature=f)


def words_of(trees, ops=OPS, F=5):
    """stage-4 words (assured id, operand word, immediate) of the trees behind each other"""
    w = [api.lower_tape_stage(*de.flatten(t, ops, np.float32), F, 4) for t in trees]
    return np.concatenate(w).astype(np.uint32) if w else np.zeros((0, 4), np.uint32)


def recount(words, F):
    """the candidates counted in Python: Counter{(operator, feature row)}"""
    c = Counter()
    for ident, arg in zip(words[:, 0].tolist(), words[:, 1].tolist()):
        if ident in PLAIN and (arg & 0xFFFFFF) < F:
            c[(PLAIN[ident], arg & 0xFFFFFF)] += 1
    return c


def expected(count, n_rows):
    return [(k, f, u) for (k, f), u in sorted(count.items(), key=lambda kv: (-kv[1], kv[0]))[:n_rows]]


def test_the_kernels_have_rows_and_the_entry_points_exist():
    assert {"de_memo_rows_max", "de_memo_rows_assign", "de_program_memo_rows", "de_program_last_memo_named"} <= set(api.EXPORTS)
    assert 2 <= api.library().de_memo_rows_max() <= api.MEMO_ROWS_MAX  # (the two loss vectors + the build's DE_MEMO_ROWS)


def test_a_unary_of_a_feature_is_a_candidate_in_both_forms():
    """cos(x2) at the start of a tree (no spill) and behind a spilled accumulator (PUSH) are both counted, for cos and for exp"""
    w = words_of([de.Node(MUL, de.Node(COS, X(2)), de.Node(COS, X(2))), de.Node(MUL, de.Node(EXP, X(4)), de.Node(EXP, X(4))),
                  de.Node(OPS.binops.index("/") + 1, de.Node(COS, X(2)), de.Node(EXP, X(4)))])
    ids = set(w[:, 0].tolist())
    assert {ta.TOPA["UNROW"] + k * 8 + push * 2 for k in (0, 1) for push in (0, 1)} <= ids, sorted(ids)
    assert api.memo_rows_assign(w, 5, 4) == [(0, 1, 3), (1, 3, 3)]


def test_ties_go_to_the_smaller_operator_then_feature():
    trees = [de.Node(ADD, de.Node(k, X(f)), X(1)) for k in (EXP, COS) for f in (5, 3, 4)] * 2
    trees += [de.Node(ADD, de.Node(COS, X(2)), X(1))] * 3
    got = api.memo_rows_assign(words_of(trees), 5, 4)
    assert got == [(0, 1, 3), (0, 2, 2), (0, 3, 2), (0, 4, 2)]
    assert api.memo_rows_assign(words_of(trees), 5, 6) == got + [(1, 2, 2), (1, 3, 2)]


def test_fewer_pairs_than_rows_and_none_at_all():
    trees = [de.Node(ADD, de.Node(EXP, X(2)), X(1)), de.Node(ADD, de.Node(EXP, X(2)), de.Node(COS, X(5)))]
    assert api.memo_rows_assign(words_of(trees), 5, 4) == [(1, 1, 2), (0, 4, 1)]
    none = [de.Node(ADD, X(1), X(2)), de.Node(COS, de.Node(MUL, X(1), X(2))), de.Node(EXP, de.Node(val=0.5))]
    assert api.memo_rows_assign(words_of(none), 5, 4) == []
    assert api.memo_rows_assign(np.zeros((0, 4), np.uint32), 5, 4) == []
    assert api.memo_rows_assign(words_of(trees), 5, 0) == []


def test_a_slot_row_is_no_candidate():
    """the operand word of a candidate names a FEATURE row: the same id on a row behind the features (a spill slot holds another value in
    every tree) is not counted, whatever its frequency"""
    w = words_of([de.Node(ADD, de.Node(COS, X(2)), X(1))])
    i = int(np.flatnonzero(w[:, 0] == ta.TOPA["UNROW"])[0])
    slot = w.copy()
    slot[i, 1] = 7  # row 7 of a 5-feature program: a spill slot
    assert api.memo_rows_assign(np.concatenate([slot] * 5 + [w]), 5, 4) == [(0, 1, 1)]


@pytest.mark.parametrize("n_rows", [1, 3, 4, 6])
def test_600_random_trees(n_rows):
    """per operator set of tests/test_assured.py's 600 trees: the assigned pairs are the most frequent ones, none twice"""
    groups = {}
    for tree, ops, F in ta.populations():
        groups.setdefault((id(ops), F), (ops, F, []))[2].append(tree)
    seen = 0
    for ops, F, trees in groups.values():
        names = list(ops.unaops)
        if "cos" not in names and "exp" not in names:
            continue
        w = words_of(trees, ops, F)
        count = recount(w, F)
        got = api.memo_rows_assign(w, F, n_rows)
        assert got == expected(count, n_rows)
        assert len({(k, f) for k, f, _ in got}) == len(got) == min(n_rows, len(count))
        rest = [u for (k, f), u in count.items() if (k, f) not in {(a, b) for a, b, _ in got}]
        assert not rest or not got or max(rest) <= min(u for _, _, u in got)
        seen += len(got)
    assert seen >= n_rows
