"""The conditions of tests/test_gpu_loss_grad_accuracy.py shown on the reference alone (no GPU).

Transparency: for every opcode and dtype the CPU oracle through each form of tests/loss_grad_accuracy.py (one tree per point, the point
in the tree's constants, every feature -0.0, N = 1, GRAD_CONSTANT) gives the BITS of the oracle on the leaf form at the same points:
values, partial rows and flags.  So an entry of the device's fused gradient under the vehicle is the kernel's partial and nothing else,
and the kept share per region is that of the population (asserted).  The reverse encoder takes every form (host-only hook), so the
device test measures the reverse kernel and not its silent fall-back.

Wrong models fail: the acceptance rule (E <= 1.01 B(x; s_device) + 2^-9 at every kept point) refuses the division partial written as
-(v * (1 / y)) (what csrc/de_rev_threaded.hip held: worst E / limit 1.09 Float32, 1.2 Float64), the two partials of a non-commutative
operator swapped, and a flipped sign; it accepts -(v / y)."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import loss_grad_accuracy as lga
import operator_accuracy as oa
from oracle import oracle

CASES = [(k, dt) for k in oa.OPS for dt in oa.DTYPES]
IDS = [f"{oa.key_name(k)}-{np.dtype(dt).name}" for k, dt in CASES]


def population_args(key, dtype):
    if key in oa.EXACT:
        args, regions, _ = oa.exact_population(key, dtype)
        return args, regions, None
    pop = oa.partial_population(key, dtype)
    return pop.args, pop.regions, pop


@pytest.mark.parametrize("key,dtype", CASES, ids=IDS)
def test_vehicle_is_transparent_on_the_oracle(key, dtype):
    args, regions, pop = population_args(key, dtype)
    out, grad, _ = oa.oracle_grad(oracle, key, args)
    for form in lga.forms(key):
        v, rows, ok = lga.oracle_form(oracle, key, form, args)
        # the leaf form's flag is one flag for the whole population; per point it is "value and every row finite"
        fin = np.isfinite(out)
        for k in range(key[1]):
            same = oa.same_bits(rows[k], grad[k])
            assert same.all(), f"{form} d{k}: {(~same).sum()} of {len(same)} rows differ, first at {[a[np.argmax(~same)] for a in args]}"
            fin &= np.isfinite(grad[k])
        same = oa.same_bits(v, out)
        assert same.all(), f"{form}: {(~same).sum()} values differ, first at {[a[np.argmax(~same)] for a in args]}"
        assert np.array_equal(ok, fin), f"{form}: {(ok != fin).sum()} flags differ from `value and rows finite`"
        if pop is not None:
            failures, maxima = lga.accept(pop, rows, pop.b_orc)
            assert not failures, f"{form}: " + "; ".join(failures)
            for k in range(key[1]):   # a kept point's tree is complete
                assert ok[pop.keep[k]].all(), (form, k)


@pytest.mark.parametrize("key,dtype", CASES, ids=IDS)
def test_reverse_encoder_takes_every_form(key, dtype):
    """encode_grad_reverse (csrc/de_grad_encode.cpp) through the host-only hook: a form it refused would run forward duals silently."""
    from dynamicexpressions_jl_amd import api
    for form in lga.forms(key):
        tape, consts = de.flatten(lga.form_tree(key, form, [1.25, 0.75, 2.5][:key[1]]), oa.operator_enum(key), dtype)
        words, _ = api.lower_tape_grad(tape, consts, lga.form_features(key, form), oracle.GRAD_CONSTANT, 3, dtype=dtype)
        assert len(words), f"{oa.key_name(key)} {form}: the reverse encoder refuses the form"
    tape, consts = de.flatten(oa.leaf_tree(key), oa.operator_enum(key), dtype)   # the sum form: leaf operands, GRAD_VARIABLE
    assert len(api.lower_tape_grad(tape, consts, key[1], oracle.GRAD_VARIABLE, 3, dtype=dtype)[0]), f"{oa.key_name(key)}: the leaf form"


@pytest.mark.parametrize("op", ["max", "min"])
def test_swapped_max_min_are_named_in_the_gradient_program(op):
    """The lowering evaluates op(leaf, subtree) as op'(subtree, leaf).  The value of max / min commutes, so the eval program keeps the
    opcode and only marks the instruction (hdr bit 16); their partials at a tie do not, so the gradient binding names the
    reversed forms DOP_RMAX = 0xF8 / DOP_RMIN = 0xF9 (found on the device by tests/test_gpu_loss_grad_accuracy.py: the tie of
    max(c1, x1 + c2) went to the first argument)."""
    from dynamicexpressions_jl_amd import api
    key, code, rcode = (op, 2), de.OPCODES[(op, 2)], {"max": 0xF8, "min": 0xF9}[op]
    for form in lga.forms(key):
        tape, consts = de.flatten(lga.form_tree(key, form, [1.25, 0.75]), oa.operator_enum(key), np.float32)
        hdr = np.asarray(api.lower_tape(tape, consts, lga.form_features(key, form))[0]).reshape(-1, 4)[:, 0]
        ops = hdr[(hdr & 0xFF) == code]
        assert len(ops) == 1 and bool(ops[0] & (1 << 16)) == (form == "const-left"), (form, [hex(int(h)) for h in hdr])
        words, _ = api.lower_tape_grad(tape, consts, lga.form_features(key, form), oracle.GRAD_CONSTANT, 3)
        assert int(((words[:, 1] >> 24) == rcode).sum()) == (1 if form == "const-left" else 0), (form, words)
    tree = de.Node(1, de.Node(feature=1), de.Node(2, de.Node(feature=2), de.Node(val=0.5)))   # op(x1, x2 + c): a feature leaf on the left
    tape, consts = de.flatten(tree, oa.operator_enum(key), np.float32)
    words, _ = api.lower_tape_grad(tape, consts, 2, oracle.GRAD_VARIABLE, 3)
    assert int(((words[:, 2] >> 24) == rcode).sum()) == 1, words


# ---- wrong models ----------------------------------------------------------------------------------------------------------------------
def _division_rows(pop, formula):
    x, y = pop.args
    with np.errstate(all="ignore"):
        v = x / y
        gl = pop.dtype(1) / y
        return gl, (-(v / y) if formula == "quotient" else -(v * gl))


@pytest.mark.parametrize("dtype", oa.DTYPES, ids=["f32", "f64"])
def test_the_rule_refuses_the_reciprocal_form_of_the_division_partial(dtype):
    pop = oa.partial_population(("/", 2), dtype)
    failures, maxima = lga.accept(pop, _division_rows(pop, "quotient"), pop.b_dev)
    assert not failures, failures
    good = max(m["worst_ratio"] for m in maxima.values())
    failures, maxima = lga.accept(pop, _division_rows(pop, "reciprocal"), pop.b_dev)
    bad = {kr: m["worst_ratio"] for kr, m in maxima.items()}
    print(f"{np.dtype(dtype).name}: -(v / y) worst E / limit {good:.3f}; -(v * (1 / y)): {bad}")
    assert failures and all(f.startswith("d1 ") for f in failures), failures   # partial 1 only: 1 / y itself is the reference's
    assert max(bad.values()) > 1.0 >= good


SWAP_CASES = [(k, dt) for k in (("/", 2), ("^", 2), ("pow_abs2", 2)) for dt in oa.DTYPES]


@pytest.mark.parametrize("key,dtype", SWAP_CASES, ids=[f"{oa.key_name(k)}-{np.dtype(dt).name}" for k, dt in SWAP_CASES])
def test_the_rule_refuses_swapped_partials_and_a_sign_flip(key, dtype):
    pop = oa.partial_population(key, dtype)
    _, grad, _ = oa.oracle_grad(oracle, key, pop.args)
    assert not lga.accept(pop, grad, pop.b_dev)[0]
    swapped, _ = lga.accept(pop, (grad[1], grad[0]), pop.b_dev)
    assert any(f.startswith("d0 ") for f in swapped) and any(f.startswith("d1 ") for f in swapped), swapped
    for k in range(2):
        flipped = tuple(-g if j == k else g for j, g in enumerate(grad))
        failures, _ = lga.accept(pop, flipped, pop.b_dev)
        assert failures and all(f.startswith(f"d{k} ") for f in failures), (k, failures)


@pytest.mark.parametrize("dtype", oa.DTYPES, ids=["f32", "f64"])
def test_a_sign_flip_of_a_unary_partial_is_refused(dtype):
    for key in (("tanh", 1), ("gamma", 1), ("atan", 1)):
        pop = oa.partial_population(key, dtype)
        _, grad, _ = oa.oracle_grad(oracle, key, pop.args)
        assert not lga.accept(pop, grad, pop.b_dev)[0]
        assert lga.accept(pop, (-grad[0],), pop.b_dev)[0]


# ---- the sum form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,dtype", CASES, ids=IDS)
def test_leaf_sum_bound_holds_for_the_oracle_and_refuses_a_swap(key, dtype):
    """The oracle's rows, summed in the working type in order and pairwise, are within the bound of the sum form; with two rows swapped
    (`/`, `^`, `-`: a misrouted partial on a leaf record) they are not."""
    cases = lga.leaf_sum_cases(key, dtype)
    regions = [name for name, _ in population_args(key, dtype)[1]]
    assert set(regions) - {c[0] for c in cases} == lga.leaf_sum_left_out(key, dtype)   # every other region has its sum form
    for name, args, parts in cases:
        _, grad, ok = oa.oracle_grad(oracle, key, args)
        assert ok, (name, "the tree of the first kept points is complete")
        sums = []
        for k, (hi, lo, slack) in enumerate(parts):
            row = grad[k].astype(dtype)
            seq = dtype(0)
            for v in row:
                seq = dtype(seq + v)
            for got in (seq, np.sum(row, dtype=dtype)):
                err, bound = lga.leaf_sum_error(got, hi, lo, slack, dtype)
                assert err <= bound, (name, k, err, bound)
            sums.append(seq)
        if key in (("/", 2), ("^", 2), ("-", 2)):
            err, bound = lga.leaf_sum_error(sums[1], *parts[0], dtype)
            assert err > bound, (name, "a swapped row passes", err, bound)
