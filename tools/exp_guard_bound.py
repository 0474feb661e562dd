#!/usr/bin/env python3
"""What the assured stream can remove, from the VALU slot table: CPU only.

For the benchmark population (seed 0xDE02) this prices every fused instruction of the guarded stream (stage 3 of
`de_lower_tape_stage`) and of the assured stream (stage 4) with `profiles/valu_slots.json` (VALU cycles of the handler each id names;
an end-fused last instruction is priced as its plain form in both) and reports, per tree-wave: the cycles of the guarded stream, the
share of each guard (validity tests: a tested handler minus its untested twin; the cos / exp pre-test and the division range test:
the guarded handler minus its form without the test), how many of each the intervals prove idle, and what each part of the pass
(`DE_ASSURED_PARTS`: 1 validity, 2 pre-tests, 4 division halves of the plain forms, 8 the TOP_BIN2 divisions + the feature bound,
16 the end-fused last instruction) removes.  `--fold` folds constant subtrees first (numpy Float32), as a program does.

`--amin A` prices the pass under the feature fact A <= |x| <= xmax (`de_lower_tape_assured_fact`: `--xmax 8 --amin 1.9073486328125e-06`
is the tight tier of a program) instead of the wide fact's lower bound (2^-39 with part 8, 2^-40 without).

    python tools/exp_guard_bound.py [--trees 1000] [--xmax 64] [--amin A] [--fold] > profiles/exp_guard_bound.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dynamicexpressions_jl_amd as de  # noqa: E402
from dynamicexpressions_jl_amd import api  # noqa: E402

BIN, UN, GEN_ROW = 5, 29, 41
LOADROW, LOADCONST_PUSH, UNROW, BINROWC, BIN2, TOP_COUNT = 48, 52, 53, 77, 89, 137


def untested(top: int) -> int:
    """The id of the same operator without any validity test (what the pass could reach at best)."""
    if BIN <= top < GEN_ROW:
        return top - ((top - BIN) & 1)
    if LOADROW <= top < LOADCONST_PUSH:
        return top - ((top - LOADROW) & 1)
    if UNROW <= top < BINROWC:
        return UNROW + ((top - UNROW) & ~5)
    if BINROWC <= top < BIN2:
        return BIN + 4 * ((top - BINROWC) >> 1)
    if BIN2 <= top < TOP_COUNT:
        return BIN2 + ((top - BIN2) & ~2)
    return top


def guard_cycles(top, cyc):
    """(validity tests, cos / exp pre-test, division range test) VALU cycles inside the guarded handler `top`."""
    val = cyc[top] - cyc[untested(top)]
    pre = div = 0.0
    k = un = None
    if BIN <= top < UN: k, cst = (top - BIN) >> 2, (top - BIN) & 2
    elif BINROWC <= top < BIN2: k, cst = (top - BINROWC) >> 1, 0
    elif BIN2 <= top < TOP_COUNT: k, cst = (top - BIN2) >> 3, (top - BIN2) & 4
    elif UN <= top < GEN_ROW: un = (top - UN) >> 2
    elif UNROW <= top < BINROWC: un = (top - UNROW) >> 3
    if k is not None and k >= 4:  # priced on the plain forms: row / row 21 -> 185, constant 23 -> 191
        div = cyc[BIN + 16 + (2 if cst else 0)] - cyc[A_DIV + (2 if cst else 0) * 3]
    if un is not None and un < 2:
        pre = cyc[UN + 4 * un] - cyc[A_UN + 4 * un]
    return val, pre, div


A_UN, A_UNROW, A_DIV, A_DIV2 = 161, 169, 185, 209  # csrc/de_bind.h TOPA_*: cos / exp without the pre-test, divisions by tested operand halves, TOP_BIN2 divisions
PARTS = (1, 2, 4, 3, 5, 7, 11, 15, 19, 27, 31)


def fold(tree, ops):
    """`tree` with every constant subtree replaced by its Float32 value (what de_program_create does before it lowers)."""
    if tree.degree == 0:
        return tree
    kids = [fold(c, ops) for c in tree.children]
    if all(k.degree == 0 and k.constant for k in kids):
        import prog_interp
        name = (ops.unaops if tree.degree == 1 else ops.binops)[tree.op - 1]
        code = de.OPCODES[(name, tree.degree)]
        fn = prog_interp.UNARY[code] if tree.degree == 1 else prog_interp.BINARY[code]
        with np.errstate(all="ignore"):
            v = np.float32(fn(*[np.array([k.val], dtype=np.float32) for k in kids])[0])
        if np.isfinite(v):
            return de.Node(val=float(v))
    return de.Node(op=tree.op, children=kids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--xmax", type=float, default=64.0)
    ap.add_argument("--amin", type=float, default=None, help="lower bound of the feature fact, amin <= |x| <= xmax (default: the wide fact's, 2^-39 / 2^-40 by parts)")
    ap.add_argument("--fold", action="store_true", help="fold constant subtrees before lowering, as a program does")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))  # (prog_interp: the numpy operators)
    os.environ["DE_ASSURED_XMAX"] = repr(args.xmax)
    with open(os.path.join(ROOT, "profiles", "valu_slots.json")) as fh:
        tab = json.load(fh)
    cyc = {int(k): v["valu_cycles"] for k, v in tab["handlers"].items()}
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(args.trees, seed=0xDE02)
    n = float(len(trees))
    over = tab["per_tree_overhead_cycles"]
    guarded = val = pre = div = 0.0
    n_instr = n_pre = n_half = 0
    bits_n = {1: 0, 2: 0, 4: 0, 8: 0, 16: 0, 32: 0, 64: 0}
    by_parts = {p: 0.0 for p in PARTS}
    n_end = end_changed = 0
    for tree in trees:
        if args.fold:
            tree = fold(tree, ops)
        tape, consts = de.flatten(tree, ops, np.float32)
        f3 = api.lower_tape_stage(tape, consts, 5, 3)
        for top in f3[:, 0]:
            g = guard_cycles(int(top), cyc)
            n_instr += 1
            guarded += cyc[int(top)]
            val, pre, div = val + g[0], pre + g[1], div + g[2]
            n_pre += g[1] > 0
            n_half += (2 if g[2] > 30 else 1) if g[2] > 0 else 0
        info = api.lower_tape_assured(tape, consts, 5, args.xmax, parts=31, amin=args.amin)  # (every part)
        for b in info[:, 5].astype(int):
            for k in bits_n:
                bits_n[k] += bool(b & k)
        g = int(f3[-1, 0])
        if len(f3) >= 2 and ((BIN <= g < UN and (g - BIN) & 1) or (UN <= g < GEN_ROW and (g - UN) & 3 == 1)):
            n_end += 1
            end_changed += int(info[-1, 4]) != g
        for p in by_parts:
            if args.amin is not None:  # (the ids of the pass under the given fact: what stage 4 / 5 of a program with that fact names)
                ids = api.lower_tape_assured(tape, consts, 5, args.xmax, parts=p, amin=args.amin)[:, 4]
            else:
                os.environ["DE_ASSURED_PARTS"] = str(p)
                ids = api.lower_tape_stage(tape, consts, 5, 4)[:, 0]
            by_parts[p] += sum(cyc[int(t)] for t in ids)
    tot = guarded + over * n
    out = {
        "source": "tools/exp_guard_bound.py: profiles/valu_slots.json over the fused programs of the bench population (seed 0xDE02, "
                  + ("constant subtrees FOLDED" if args.fold else "UNFOLDED tapes as de_lower_tape_stage lowers them") +
                  "; an end-fused last instruction priced as its plain form in both streams — the end-fused twins have no stream id and no "
                  "entry in the slot table, so what part 16 removes is priced by the guards of the plain forms: a proxy)",
        "trees": len(trees), "xmax": args.xmax, "amin": args.amin,
        "fused_instructions_per_tree": n_instr / n,
        "valu_cycles_per_tree_wave_guarded": tot / n,
        "guards_share_of_guarded": {"validity_tests": val / tot, "cos_exp_pre_tests": pre / tot, "division_range_tests": div / tot,
                                    "all": (val + pre + div) / tot},
        "guards_per_tree": {"cos_exp_pre_tests": n_pre / n, "division_operand_halves": n_half / n},
        "elided_per_tree": {"validity_result": bits_n[1] / n, "validity_row": bits_n[2] / n, "cos_exp_pre_tests": bits_n[4] / n,
                            "division_halves_accumulator": bits_n[8] / n, "division_halves_row": bits_n[16] / n,
                            "division_halves_bin2_row_a": bits_n[32] / n, "division_halves_bin2_row_b": bits_n[64] / n},
        "end_fused_trees_share": n_end / n, "end_fused_with_an_assured_twin_share": end_changed / n,
        "provably_idle_share": {"cos_exp_pre_tests": bits_n[4] / max(n_pre, 1), "division_operand_halves": (bits_n[8] + bits_n[16] + bits_n[32] + bits_n[64]) / max(n_half, 1)},
        "removed_share_of_guarded_by_DE_ASSURED_PARTS": {str(p): (guarded - c) / tot for p, c in sorted(by_parts.items())},
        "removed_cycles_per_tree_wave_by_DE_ASSURED_PARTS": {str(p): (guarded - c) / n for p, c in sorted(by_parts.items())},
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
