"""CPU unit tests of the two gradient stream encoders (csrc/de_grad_encode.cpp) through the host-only hook ``de_lower_tape_grad``: the
hook encodes against an identity handler table, so a record's handler word is a plain ``gop_*`` / ``ROP_*`` id of csrc/de_bind.h.  What
is asserted holds by construction — the id formulas and field layouts of de_bind.h, restated below — never a recorded stream."""
import struct

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api

N = de.Node
OPS = de.synth.BENCH_OPERATORS  # binary + - / *, unary cos exp
VARIABLE, CONSTANT, BOTH = 0, 1, 2
LEAF, SLOT, CONST, ACC = 0, 1, 2, 3


# ---- csrc/de_bind.h: handler ids of the threaded gradient kernel, window width GC ---------------------------------------------------
class Gop:
    def __init__(self, GC):
        self.ns = ns = GC + 2
        self.push, self.check_acc, self.bin_base = 2 * ns + 1, 2 * ns + 2, 2 * ns + 3
        self.un_base = self.bin_base + 2 * 8 * (2 * ns + 1)
        self.gen_base = self.un_base + 2 * 13 * (ns + 2)
        self.param, self.tern, self.pushload_base = self.gen_base + 4, self.gen_base + 5, self.gen_base + 6
        self.count = self.gen_base + 6 + 2 * ns

    def load(self, src, sv=0):
        return sv if src == LEAF else (self.ns if src == SLOT else self.ns + 1 + sv)

    def bin(self, k, src, sv, chk):
        return self.bin_base + (k * 2 + chk) * (2 * self.ns + 1) + self.load(src, sv)

    def un(self, k, src, sv, chk):
        return self.un_base + (k * 2 + chk) * (self.ns + 2) + (sv if src == LEAF else (self.ns if src == SLOT else self.ns + 1))

    def pushload(self, src, sv):
        return self.pushload_base + (0 if src == LEAF else self.ns) + sv

    def operands(self, g):
        """(what the operand word names: 'leaf' | 'slot' | None, carries a constant's bits, lo is a byte distance to a slot)"""
        ns = self.ns
        pick = lambda i: ("leaf", False) if i < ns else (("slot", False) if i == ns else (None, True))
        if g < self.push:
            return (*pick(g), False)
        if g == self.push:
            return "slot", False, False
        if g < self.bin_base:
            return None, False, False
        if g < self.un_base:
            return (*pick((g - self.bin_base) % (2 * ns + 1)), False)
        if g < self.gen_base:
            i = (g - self.un_base) % (ns + 2)
            return ("leaf" if i < ns else ("slot" if i == ns else None)), False, False
        if g < self.param:
            return [("leaf", False, False), ("slot", False, False), (None, True, False), (None, False, False)][g - self.gen_base]
        if g == self.param:
            return None, False, False
        if g == self.tern:
            return "slot", False, True
        i = g - self.pushload_base
        return ("leaf", False, True) if i < ns else ("slot", True, False)


# ---- csrc/de_bind.h: RevOp ---------------------------------------------------------------------------------------------------------------
R_PUSH, R_CHECK, R_BIN, R_UN, R_GEN, R_TERN, R_PARAM = 3, 4, 5, 53, 105, 109, 110
R_R_UN, R_R_NEG, R_R_POP, R_R_LEAF, R_R_BIN, R_R_TERN = 111, 112, 113, 114, 115, 123
R_F_PUSHLOAD, R_F_PUSHUN, R_R_LEAFX, R_R_BINCOLX, R_UN_SLOT, R_R_SLOTACC, R_R_BINACC, R_R_POPADD, R_COUNT = 124, 126, 152, 156, 164, 190, 192, 196, 197
rop_bin = lambda k, src, chk: R_BIN + (k * 3 + src) * 2 + chk
rop_rbin = lambda pk, ok: R_R_BIN + pk * 2 + ok
rop_bincolx = lambda pk, pop: R_R_BINCOLX + pk * 2 + pop


def rev_offsets(r, rec):
    """(LDS byte offsets, LDS row indices, carries a constant's bits) of the reverse record `rec` under handler id r"""
    _, arg, lo, hi = (int(v) for v in rec)
    low = lambda w: w & 0xFFFFFF
    colrows = lambda w: [(w >> 16) & 0x3FFF] if w >> 30 else []  # column word: [29:16] accumulation row unless "reduce now"
    if r in (0, 1, R_PUSH, R_R_POP, R_R_POPADD, R_R_UN) or R_R_SLOTACC <= r < R_R_BINACC:
        return [arg], [], False
    if r == 2:
        return [], [], True
    if R_BIN <= r < R_UN:
        src = ((r - R_BIN) // 2) % 3
        return ([arg], [], True) if src == CONST else ([arg, lo], [], False)
    if R_UN <= r < R_GEN:
        return ([arg, lo], [], False) if ((r - R_UN) // 2) % 2 else ([arg], [], False)
    if R_GEN <= r < R_TERN:
        src = r - R_GEN
        return ([arg, low(lo)], [], False) if src in (LEAF, SLOT) else ([low(arg)], [], src == CONST)
    if r in (R_TERN, R_R_TERN):
        return [low(arg)], [lo & 0xFFFF, lo >> 16], False
    if r == R_R_LEAF:
        return [], colrows(lo), False
    if R_R_BIN <= r < R_R_TERN:
        return ([arg, lo], [], False) if (r - R_R_BIN) % 2 == 0 else ([arg], colrows(lo), False)
    if r == R_F_PUSHLOAD:
        return [arg & 0xFFFF, arg >> 16], [], False
    if r == R_F_PUSHLOAD + 1:
        return [arg], [], True
    if R_F_PUSHUN <= r < R_R_LEAFX:
        return [arg & 0xFFFF, arg >> 16, lo], [], False
    if R_R_LEAFX <= r < R_R_BINCOLX:
        return [arg & 0xFFFF, arg >> 16], colrows(lo), False
    if R_R_BINCOLX <= r < R_UN_SLOT:
        return [arg & 0xFFFF, arg >> 16], colrows(lo) + colrows(hi), False
    if R_UN_SLOT <= r < R_R_SLOTACC:
        return [arg, lo], [], False
    if R_R_BINACC <= r < R_R_POPADD:
        return [arg, lo], [], False
    return [], [], False  # CHECK, PARAM, R_NEG


def unrotate(ids, chains):
    """The handler word of a record names the handler of the record BEHIND it, a chain's last record the chain's first."""
    out = np.array(ids)
    for a, b in chains:
        if b - a >= 2:
            out[a + 1:b] = ids[a:b - 1]
            out[a] = ids[b - 1]
    return out


def bits(consts, dtype):
    return [struct.unpack("<II", struct.pack("<d", float(c))) if dtype == np.float64 else (struct.unpack("<I", struct.pack("<f", float(c)))[0], None)
            for c in consts]


def imm(rec, dtype):
    return (int(rec[2]), int(rec[3])) if dtype == np.float64 else (int(rec[2]), None)


def population():
    """A few dozen seeded trees: the bench operator set, parametric ones, and 12 features (several windows, Float64 included)."""
    items = [(t, 5, 0) for t in de.synth.random_population(24, seed=0xE17C)]
    items += [(t, 5, 2) for t in de.synth.random_population(8, seed=0xE17D, node_type=de.ParametricNode, nparams=2)]
    items += [(t, 12, 0) for t in de.synth.random_population(8, seed=0xE17E, nfeatures=12)]
    return items


POPULATION = population()


def bound_consts(tape, consts, F, P, dtype):
    """The constants' bits in PROGRAM order: the constant-source records of the bound program (stage 2, early-exit binding)."""
    b = api.lower_tape_stage(tape, consts, F, 2, P, 7, dtype)
    is_const = lambda bop: bop in (1, 42) or (5 <= bop < 29 and (bop - 5) & 2)  # LOAD_CONST, GEN_CONST, the hot binary block's constant forms
    return [imm(r, dtype) for r in b if is_const(int(r[0]))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", [VARIABLE, CONSTANT, BOTH])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_forward_streams_hold_what_the_kernel_relies_on(dtype, mode, form):
    es = np.dtype(dtype).itemsize
    n_streams = 0
    for tree, F, P in POPULATION:
        tape, consts = de.flatten(tree, OPS, dtype)
        _, lmeta = api.lower_tape(tape, consts, F, P, 7, dtype)
        w, meta = api.lower_tape_grad(tape, consts, F, mode, form, P, 7, dtype)
        if len(w) == 0:
            continue  # (Float64 has no module for 6 .. 8 rows: the flat kernel runs those trees)
        n_streams += 1
        GC, VS, windows, slots, n0, variants = (int(v) for v in meta[:6])
        assert variants == (4 if form == 2 else 1) and len(w) == n0 * variants and (VS == 1 or (form == 1 and dtype == np.float32))
        G = {VARIABLE: F + P, CONSTANT: len(consts), BOTH: F + P + len(consts)}[mode]
        assert windows * GC >= G
        g = Gop(GC)
        RB, FE = 64 * VS * es, F + (P if lmeta["uses_params"] else 0)
        slot_rows = max(slots * (1 + GC), GC)
        rows = FE + variants * slot_rows  # what the launch allocates per wave (shared leaf rows: once + four slot areas)
        ids = unrotate(w[:n0, 0], [(0, n0)])
        assert (w[:, 0] < g.count).all()
        assert ids[-1] == g.param and (ids == g.param).sum() == 1
        carried = []
        for v in range(variants):
            shift = v * slot_rows * RB
            for j in range(n0):
                rec, rec0 = w[v * n0 + j], w[j]
                what, has_const, lo_dist = g.operands(int(ids[j]))
                off = int(rec[1]) & 0xFFFFFF
                if what == "leaf":
                    assert off % RB == 0 and off < FE * RB
                elif what == "slot":
                    assert off % RB == 0 and FE * RB + shift <= off < (FE + slot_rows) * RB + shift
                if lo_dist:
                    second = off + int(rec[2])
                    assert second % RB == 0 and FE * RB + shift <= second < (FE + slot_rows) * RB + shift and second < rows * RB
                if has_const and v == 0:
                    carried.append(imm(rec, dtype))
                # a stream variant = variant 0, but for the slot bytes of wave v on the records that name a slot
                want = rec0.copy()
                if what == "slot":
                    want[1] += shift
                elif lo_dist:
                    want[2] += shift
                assert (rec == want).all()
        assert carried == bound_consts(tape, consts, F, P, dtype) and sorted(carried) == sorted(bits(consts, dtype))
        assert meta[6] == len(consts)
    assert n_streams >= (12 if dtype == np.float64 else 30)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", [VARIABLE, CONSTANT, BOTH])
def test_reverse_streams_hold_what_the_kernel_relies_on(dtype, mode):
    RB = 64 * np.dtype(dtype).itemsize
    for tree, F, P in POPULATION:
        tape, consts = de.flatten(tree, OPS, dtype)
        w, meta = api.lower_tape_grad(tape, consts, F, mode, 3, P, 7, dtype)
        mid, need, stage_cols, rows, n_slots = (int(v) for v in meta[:5])
        n = len(w)
        assert n > 0 and 0 < mid < n and stage_cols >= 64 and rows * RB * 4 <= 160 * 1024
        assert (w[:, 0] < R_COUNT).all()
        ids = unrotate(w[:, 0], [(0, mid), (mid, n)])
        assert list(np.flatnonzero(ids == R_PARAM)) == [mid - 1, n - 1]  # the end records of the two sweeps, nowhere else
        carried = []
        for j in range(n):
            offs, idx, has_const = rev_offsets(int(ids[j]), w[j])
            assert all(o % RB == 0 and o < rows * RB for o in offs), (j, int(ids[j]), offs)
            assert all(i < rows for i in idx)
            if has_const:
                carried.append(imm(w[j], dtype))
        assert carried == bound_consts(tape, consts, F, P, dtype) and sorted(carried) == sorted(bits(consts, dtype))
        assert meta[6] == len(consts)


def words_of(tree, mode, form, F=2, dtype=np.float32, ops=OPS):
    tape, consts = de.flatten(tree, ops, dtype)
    w, meta = api.lower_tape_grad(tape, consts, F, mode, form, 0, 7, dtype)
    return [[int(v) for v in r] for r in w], meta


def test_known_answers_of_the_smallest_forward_streams():
    """Two features, Float32 (one wave's row: 256 bytes), derived by hand from the id formulas.  Records are listed in program order with
    their OWN handler; the stream holds them successor-rotated."""
    x1, x2, c = N(feature=1), N(feature=2), N(val=2.5)
    C = 0x40200000  # 2.5f

    def expect(tree, mode, natural):
        w, meta = words_of(tree, mode, 0)
        ids = [r[0] for r in natural]
        assert w == [[ids[(j + 1) % len(ids)]] + r[1:] for j, r in enumerate(natural)]
        return meta

    g2, g1, g3 = Gop(2), Gop(1), Gop(3)
    # x1 alone.  VARIABLE: two rows -> window 2, x1 seeds row 0: the leaf load of seed variant 2 + 0.  CONSTANT: no row -> window 1, no seed
    meta = expect(x1, VARIABLE, [[g2.load(LEAF, 2), 0, 0, 0], [g2.param, 0, 0, 0]])
    assert list(meta[:6]) == [2, 1, 1, 0, 2, 1]
    expect(x1, CONSTANT, [[g1.load(LEAF, 1), 0, 0, 0], [g1.param, 0, 0, 0]])
    # x1 + c, validity-tested: the constant seeds row 0 in CONSTANT mode (variant 2 + 0), nothing in VARIABLE mode (variant 1)
    expect(N(1, x1, c), CONSTANT, [[g1.load(LEAF, 1), 0, 0, 0], [g1.bin(0, CONST, 2, True), 0, C, 0], [g1.param, 0, 0, 0]])
    expect(N(1, x1, c), VARIABLE, [[g2.load(LEAF, 2), 0, 0, 0], [g2.bin(0, CONST, 1, True), 0, C, 0], [g2.param, 0, 0, 0]])
    # ... and row F + 0 = 2 of three in BOTH mode
    expect(N(1, x1, c), BOTH, [[g3.load(LEAF, 2), 0, 0, 0], [g3.bin(0, CONST, 4, True), 0, C, 0], [g3.param, 0, 0, 0]])
    # cos(c): load, then the hot unary handler on the accumulator — two records for one bound record, the constant in the first
    meta = expect(N(1, N(val=0.5)), CONSTANT, [[g1.load(CONST, 2), 0, 0x3F000000, 0], [g1.un(0, ACC, 0, False), 0, 0, 0], [g1.check_acc, 0, 0, 0],
                                                [g1.param, 0, 0, 0]])
    assert meta[6] == 1
    # x1 * x2: the second operand straight from its row (byte 256), seeding row 1
    expect(N(4, x1, x2), VARIABLE, [[g2.load(LEAF, 2), 0, 0, 0], [g2.bin(3, LEAF, 3, True), 256, 0, 0], [g2.param, 0, 0, 0]])
    # (x1 + x2) * (x1 - x2), the smallest product that spills: x1 - x2 first, then PUSH + LOAD x1 as ONE record (gop_pushload: operand = the
    # leaf, immediate = byte distance to the slot, which follows the two feature rows), x1 + x2, times the slot
    meta = expect(N(4, N(1, x1, x2), N(2, x1, x2)), VARIABLE,
                  [[g2.load(LEAF, 2), 0, 0, 0], [g2.bin(1, LEAF, 3, False), 256, 0, 0], [g2.pushload(LEAF, 2), 0, 512, 0],
                   [g2.bin(0, LEAF, 3, False), 256, 0, 0], [g2.bin(3, SLOT, 0, True), 512, 0, 0], [g2.param, 0, 0, 0]])
    assert list(meta[:6]) == [2, 1, 1, 1, 6, 1]


def test_known_answer_of_the_smallest_reverse_stream():
    """x1 * c in BOTH mode, Float32, two features: rows 0 .. 1 are X, the product's two partial rows follow (byte 512).  Forward: load x1,
    multiply by the constant (hot binary 3, constant operand, tested; operand word = its partial rows), end.  Backward: r_bin<partial rows,
    column> of the constant (column 1 + 2 + 0 = 3) and r_leaf of x1 (column 1 + 0, its only leaf: reduced at once) fuse into r_bincolx."""
    w, meta = words_of(N(4, N(feature=1), N(val=2.5)), BOTH, 3)
    natural = [[0, 0, 0, 0], [rop_bin(3, CONST, True), 512, 0x40200000, 0], [R_PARAM, 0, 0, 0],
               [rop_bincolx(0, False), 512, 3, 1], [R_PARAM, 0, 0, 0]]
    assert w == [[natural[[1, 2, 0, 4, 3][j]][0]] + r[1:] for j, r in enumerate(natural)]
    assert list(meta[:5]) == [3, 2, 64, 2 + 2 + 1, 0] and meta[6] == 1
    # DE_GRAD_CONSTANT: x1 has no column, the backward sweep is the unfused r_bin<partial rows, column 1> alone
    w, _ = words_of(N(4, N(feature=1), N(val=2.5)), CONSTANT, 3)
    assert [r[1:] for r in w[3:]] == [[512, 1, 0], [0, 0, 0]] and [w[4][0], w[3][0]] == [rop_rbin(0, 1), R_PARAM]


def test_trees_without_a_threaded_form_return_no_words():
    """More than 240 gradient rows (they travel in 8 bits) and, for reverse accumulation, a ternary operator on a CSE tape.  The third
    refusal of the encoders — a ternary operator one of whose first two operands is a LEAF row — cannot be reached from a tape: the
    lowering spills both operands of every ternary operator (de_bind.cpp binds the second from a slot, de_lower.cpp pushes the first),
    which the last assertions pin: the forward stream of fma(x1, x2, x3) exists and its ternary record names two slot rows."""
    x = lambda k: N(feature=k)
    tape, consts = de.flatten(x(1), OPS, np.float32)
    # (with shared leaf rows — form 2 — 240 feature rows fit the LDS: the refusal of 241 is the row count's, not the memory's)
    assert len(api.lower_tape_grad(tape, consts, 241, VARIABLE, 2)[0]) == 0
    assert len(api.lower_tape_grad(tape, consts, 241, VARIABLE, 0)[0]) == 0
    w, meta = api.lower_tape_grad(tape, consts, 240, VARIABLE, 2)
    assert len(w) == 4 * 2 and list(meta[:3]) == [8, 1, 30]
    tern = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",), ternary_operators=("fma",))
    G = de.GraphNode
    s = G(2, G(feature=1), G(feature=2))  # a shared product under a ternary operator: a CSE tape
    _, consts, cse, _ = de.flatten_graph(G(1, s, G(1, G(1, s), G(1, G(feature=1)), G(1, G(feature=2)))), tern, np.float32)
    assert cse is not None
    assert len(api.lower_tape_grad(cse, consts, 3, VARIABLE, 3)[0]) == 0
    assert len(api.lower_tape_grad(cse, consts, 3, VARIABLE, 0)[0]) > 0  # (forward duals take it)
    tape, consts = de.flatten(N(1, x(1), x(2), x(3)), tern, np.float32)
    assert len(api.lower_tape_grad(tape, consts, 3, VARIABLE, 3)[0]) > 0  # (no sharing: reverse accumulation takes the ternary operator)
    w, meta = api.lower_tape_grad(tape, consts, 3, VARIABLE, 0)
    g, RB = Gop(int(meta[0])), 256
    ids = unrotate(w[:, 0], [(0, len(w))])
    (j,) = np.flatnonzero(ids == g.tern)
    first, second = int(w[j][1]) & 0xFFFFFF, (int(w[j][1]) & 0xFFFFFF) + int(w[j][2])
    assert first % RB == 0 and second % RB == 0 and 3 * RB <= first < second < (3 + int(meta[3]) * (1 + int(meta[0]))) * RB


def test_the_hook_takes_the_real_compute_types_only():
    lib = api.library()
    tape, consts = de.flatten(N(feature=1), OPS, np.float32)
    meta = np.zeros(8, dtype=np.int32)
    for code in (2, 3, 4, 99):  # DE_F16, DE_CF32, DE_CF64, nonsense
        assert lib.de_lower_tape_grad(code, tape.ctypes.data, len(tape), None, 0, 1, 0, 7, 0, 0, None, 0, meta.ctypes.data) == -1
    assert lib.de_lower_tape_grad(0, tape.ctypes.data, len(tape), None, 0, 1, 0, 7, 3, 0, None, 0, meta.ctypes.data) == -1  # bad mode
    assert lib.de_lower_tape_grad(0, tape.ctypes.data, len(tape), None, 0, 1, 0, 7, 0, 4, None, 0, meta.ctypes.data) == -1  # bad form
