# runtests_hip.jl — what a maintainer with Julia, DynamicExpressions.jl and an MI355X runs to close SURVEY.md §8f-2:
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> runtests_hip.jl
#
# The builder's image has no Julia: this file (like the shim it loads) was never executed there.  It checks the shim
# against the REAL reference — DynamicExpressions.jl's own CPU `eval_tree_array` / `eval_grad_tree_array` on the same
# (tree, X) — which is the parity the C restatement under oracle/ can only approximate:
#   1. the 118 known answers transcribed from the reference's tests and docs (golden_cases.jl, generated from
#      tests/golden/reference_known_answers.json): flag, values at the case's tolerance, AND agreement with the CPU path
#      (1e-5 relative Float32 / 1e-12 Float64 on the samples where both are finite; identical `complete`);
#   2. a random population through HIPPopulation against the CPU path tree by tree;
#   3. GraphNode trees with shared subtrees (the CSE tape: ADVICE r2 — `flatten_cse!` threw a KeyError before round 3);
#   4. forward-mode gradients in the three modes.
using Test
using DynamicExpressions
using DynamicExpressions: Node, GraphNode, OperatorEnum, EvalContext, eval_tree_array, eval_grad_tree_array

include(joinpath(@__DIR__, "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt
include(joinpath(@__DIR__, "golden_cases.jl"))

# ---- the helper operators the reference's tests define (test/test_params.jl:7-29 and friends), registered by identity ----
safe_log(x::T) where {T} = x > zero(T) ? log(x) : T(NaN)
safe_log2(x::T) where {T} = x > zero(T) ? log2(x) : T(NaN)
safe_log10(x::T) where {T} = x > zero(T) ? log10(x) : T(NaN)
safe_sqrt(x::T) where {T} = x >= zero(T) ? sqrt(x) : T(NaN)
safe_acosh(x::T) where {T} = x >= one(T) ? acosh(x) : T(NaN)
relu(x::T) where {T} = x < zero(T) ? zero(T) : x
square(x) = x * x
cube(x) = x * x * x
neg(x) = -x
custom_cos(x) = cos(x)^2
pow_abs2(x, y) = exp(y * log(abs(x)))
for (f, n) in ((safe_log, :safe_log), (safe_log2, :safe_log2), (safe_log10, :safe_log10), (safe_sqrt, :safe_sqrt),
               (safe_acosh, :safe_acosh), (relu, :relu), (square, :square), (cube, :cube), (neg, :neg),
               (custom_cos, :custom_cos), (pow_abs2, :pow_abs2))
    HIP.register_hip_opcode(f, n)
end
const NAMED = Dict{String,Any}(
    "cos" => cos, "sin" => sin, "exp" => exp, "abs" => abs, "sqrt" => sqrt, "+" => +, "-" => -, "*" => *, "/" => /, "^" => ^,
    "max" => max, "min" => min, "rem" => rem, "fma" => fma, "clamp" => clamp, "safe_log" => safe_log, "safe_log2" => safe_log2,
    "safe_log10" => safe_log10, "safe_sqrt" => safe_sqrt, "safe_acosh" => safe_acosh, "relu" => relu, "square" => square,
    "cube" => cube, "neg" => neg, "custom_cos" => custom_cos, "pow_abs2" => pow_abs2,
)

function operators_of(case)
    names = (case.unary, case.binary, case.ternary)
    all(n -> haskey(NAMED, n), Iterators.flatten(names)) || return nothing   # (gamma: SpecialFunctions, optional)
    una = Tuple(NAMED[n] for n in case.unary)
    bin = Tuple(NAMED[n] for n in case.binary)
    ter = Tuple(NAMED[n] for n in case.ternary)
    return isempty(ter) ? OperatorEnum(1 => una, 2 => bin) : OperatorEnum(1 => una, 2 => bin, 3 => ter)
end

# S-expression -> Node{T,D} (degree D = 2, or 3 when the case has ternary operators)
function build(s, ::Type{T}, case, ::Val{D}, ::Type{N}=Node) where {T,D,N}
    s isa Number && return N{T,D}(; val=T(s))
    head = s[1]
    if head == "x" && length(s) == 2 && s[2] isa Integer
        return N{T,D}(; feature=Int(s[2]))
    end
    kids = [build(c, T, case, Val(D), N) for c in s[2:end]]
    names = (case.unary, case.binary, case.ternary)[length(kids)]
    op = findfirst(==(head), names)
    return N{T,D}(; op=op, children=Tuple(kids))
end
has_param(s) = !(s isa Number) && ((s[1] == "p" && length(s) == 2 && s[2] isa Integer) || any(has_param, s[2:end]))

matrix(::Type{T}, rows) where {T} = isempty(rows) ? zeros(T, 0, 0) : T[T(rows[f][j]) for f in 1:length(rows), j in 1:length(rows[1])]

function agree(a::AbstractVector{T}, b::AbstractVector{T}) where {T}
    rel = T === Float32 ? 1e-5 : 1e-12
    for (x, y) in zip(a, b)
        (isfinite(x) && isfinite(y)) || continue
        abs(Float64(x) - Float64(y)) <= rel * abs(Float64(y)) + 1e-30 || return false
    end
    return true
end

@testset "known answers of the reference through the HIP shim" begin
    n_run = 0
    for case in GOLDEN_CASES
        case.kind in ("eval", "flag", "grad") || continue          # (ParametricExpression: see the population tests below)
        has_param(case.tree) && continue
        ops = operators_of(case)
        ops === nothing && continue
        T = case.dtype == "float32" ? Float32 : Float64
        D = isempty(case.ternary) ? 2 : 3
        tree = build(case.tree, T, case, Val(D))
        X = matrix(T, case.X)
        ctx = EvalContext(; early_exit=Val(case.early_exit), bumper=Val(false))   # the Bumper FLAG semantics are covered in Python
        case.bumper && continue
        if case.kind == "grad"
            variable = case.mode == "variable" ? Val(true) : case.mode == "both" ? Val(:both) : Val(false)
            y, g, ok = HIP._hip_eval_grad_tree_array(tree, X, ops; variable)
            yr, gr, okr = eval_grad_tree_array(tree, X, ops; variable)
            @test ok == okr == case.ok
            if ok
                @test agree(y, yr)
                @test all(k -> agree(view(g, k, :), view(gr, k, :)), axes(g, 1))
            end
        else
            r = HIP._hip_eval_tree_array(tree, X, ops, ctx)
            @test r !== nothing
            y, ok = r
            yr, okr = eval_tree_array(tree, X, ops; eval_context=ctx)
            @test ok == case.ok
            @test ok == okr
            if ok
                @test agree(y, yr)
                if case.y !== nothing
                    want = Float64[v for v in case.y]
                    for j in eachindex(want)
                        (j - 1) in case.y_nonfinite_idx && (@test !isfinite(y[j]); continue)
                        isfinite(want[j]) || continue
                        @test abs(Float64(y[j]) - want[j]) <= max(case.atol, 1e-30) + max(case.rtol, T === Float32 ? 1e-5 : 1e-13) * abs(want[j])
                    end
                end
            end
        end
        n_run += 1
    end
    @test n_run >= 90
end

@testset "a random population: HIPPopulation against the reference CPU path" begin
    ops = OperatorEnum(1 => (cos, exp), 2 => (+, -, /, *))          # benchmark/benchmarks.jl:32-35
    for T in (Float32, Float64)
        x = [Node{T}(; feature=i) for i in 1:5]
        trees = Node{T,2}[
            x[1] * cos(x[2] - T(3.2)),                                # README.md:30-39
            exp(x[3]) / (x[4] * x[4] + T(1.5)),
            cos(exp(x[1] * T(0.3))) - x[5] * (x[2] + T(0.25)),
            x[1] / (x[2] - x[2]),                                     # 1 / 0: incomplete
            exp(exp(x[3] * T(40))),                                   # overflows: incomplete
        ]
        X = randn(T, 5, 4099)
        pop = HIP.HIPPopulation(trees, ops, 5)
        out, ok = HIP.eval_population(pop, X)
        for (t, tree) in enumerate(trees)
            yr, okr = eval_tree_array(tree, X, ops)
            @test ok[t] == okr
            okr && @test agree(view(out, :, t), yr)
        end
        @test ok == [true, true, true, false, false]
    end
end

@testset "GraphNode: shared subtrees through the CSE tape" begin
    ops = OperatorEnum(1 => (cos, exp), 2 => (+, -, /, *))
    for T in (Float32, Float64)
        x1, x2 = GraphNode{T}(; feature=1), GraphNode{T}(; feature=2)
        c = GraphNode{T}(; val=T(0.75))
        s = cos(x1 * c)                                               # ONE node object ...
        g1 = s + s * (c * x2)                                         # ... used twice; c three times
        g2 = exp(s) / (s + T(2))
        g3 = x1 * x2 + c                                              # nothing shared
        X = randn(T, 2, 1031)
        pop = HIP.HIPPopulation([g1, g2, g3], ops, 2)                 # threw KeyError in flatten_cse! before round 3
        out, ok = HIP.eval_population(pop, X)
        for (t, g) in enumerate((g1, g2, g3))
            yr, okr = eval_tree_array(g, X, ops)
            @test ok[t] == okr == true
            @test agree(view(out, :, t), yr)
        end
    end
end

@testset "forward-mode gradients in the three modes" begin
    ops = OperatorEnum(1 => (cos, exp), 2 => (+, -, /, *))
    x = [Node{Float64}(; feature=i) for i in 1:3]
    tree = x[1] * cos(x[2] * 0.7 - 3.2) + exp(x[3] * 0.1) / (x[1] * x[1] + 2.5)
    X = randn(Float64, 3, 257)
    for variable in (Val(true), Val(false), Val(:both))
        y, g, ok = HIP._hip_eval_grad_tree_array(tree, X, ops; variable)
        yr, gr, okr = eval_grad_tree_array(tree, X, ops; variable)
        @test ok == okr == true
        @test size(g) == size(gr)
        @test agree(y, yr)
        @test all(k -> agree(view(g, k, :), view(gr, k, :)), axes(g, 1))
    end
end

@testset "early exit: rows of incomplete trees are NaN, full_eval=true evaluates them (ABI version 2)" begin
    @test ccall((:de_abi_version, HIP.LIBDE), Cint, ()) == HIP.DE_HIP_ABI_VERSION
    ops = OperatorEnum(1 => (cos, exp), 2 => (+, -, /, *))
    x1, x2 = Node{Float32}(; feature=1), Node{Float32}(; feature=2)
    good = x1 * cos(x2 - 3.2f0)
    bad = exp(exp(x1 * 40.0f0)) + x2            # overflows on most samples: complete == false
    X = randn(Float32, 2, 70_001)               # several hundred sample tiles: the exit really happens
    for full_eval in (false, true)
        pop = HIP.HIPPopulation([good, bad], ops, 2; full_eval)
        out, ok = HIP.eval_population(pop, X)
        yr, okr = eval_tree_array(good, X, ops)
        @test ok == [true, false] && okr
        @test agree(view(out, :, 1), yr)        # the complete tree does not depend on the option
        if full_eval                            # every sample evaluated: the finite samples carry their values
            yb, _ = eval_tree_array(bad, X, ops; eval_context=EvalContext(; early_exit=false))
            fin = isfinite.(yb)
            @test any(fin) && agree(view(out, :, 2)[fin], yb[fin])
        else                                    # host arrays: the library NaN-fills the rows of incomplete trees
            @test all(isnan, view(out, :, 2))
        end
    end
    y1, ok1 = HIP._hip_eval_tree_array(bad, X, ops, EvalContext())
    @test !ok1 && all(isnan, y1)
end

@testset "GraphNode: a shared CONSTANT is one constant (fan-out of set_population_constants!, summed gradient rows)" begin
    # src/NodeUtils.jl:43-51 (count_constant_nodes with f_on_shared), :184-201 (the shared NodeIndex entry): the library keeps one
    # slot per occurrence, the shim fans values out and sums the occurrence rows (round 5: `occ` of HIPPopulation, combine_rows)
    ops = OperatorEnum(1 => (cos, exp), 2 => (+, -, /, *))
    x1, x2 = GraphNode{Float64}(; feature=1), GraphNode{Float64}(; feature=2)
    c = GraphNode{Float64}(; val=0.7)
    g = (x1 * c) + cos(c * x2)                  # ONE constant, two occurrences
    t2 = Node{Float64}(; feature=1) * 1.5 - 0.25  # a plain tree with two constants of its own: per-tree slot numbering
    X = randn(Float64, 2, 1_000)
    y = randn(Float64, 1_000)
    pop = HIP.HIPPopulation([g, t2], ops, 2)
    @test pop.n_consts == [1, 2] && pop.n_slots == [2, 2]
    out, ok = HIP.eval_population(pop, X)
    @test all(ok) && agree(view(out, :, 1), eval_tree_array(g, X, ops)[1]) && agree(view(out, :, 2), eval_tree_array(t2, X, ops)[1])
    lossv, dl, okl = HIP.eval_population_loss_grad(pop, X, y)
    @test length(dl[1]) == 1 && length(dl[2]) == 2
    _, gr, _ = eval_grad_tree_array(g, X, ops; variable=Val(false))      # 1 x N: the shared constant's single row
    yg, _ = eval_tree_array(g, X, ops)
    @test isapprox(dl[1][1], sum(2 .* (yg .- y) .* view(gr, 1, :)); rtol=1e-9)
    HIP.set_population_constants!(pop, [0.3, 2.0, -1.0])                 # g's constant, then t2's two
    c.val = 0.3
    out2, _ = HIP.eval_population(pop, X)
    @test agree(view(out2, :, 1), eval_tree_array(g, X, ops)[1])
    @test agree(view(out2, :, 2), X[1, :] .* 2.0 .- (-1.0))
    _, gm, _ = HIP._hip_eval_grad_tree_array(g, X, ops; variable=Val(false))
    @test size(gm, 1) == 1
end

@testset "round 6 / ABI 3: strict flags, the reverse-accumulation opt-in, trim" begin
    # (a) eval_population_strict: outside `uncertified` the flag IS the reference's `complete` — including the isfinite(sum(x)) quirk
    #     (src/ValueInterface.jl:9): ((x1 + 2.5) * big) / big has finite elements and an overflowing SUM
    ops = OperatorEnum(1 => (cos, exp), 2 => (+, -, /, *))
    x1 = Node{Float32}(; feature=1)
    big = 3.0f34
    quirk = ((x1 + 2.5f0) * big) / big
    plain = x1 * cos(x1 - 3.2f0)
    X = abs.(randn(Float32, 2, 4096)) .+ 0.5f0
    pop = HIP.HIPPopulation([quirk, plain], ops, 2)
    out, ok, uncertified = HIP.eval_population_strict(pop, X)
    @test 1 in uncertified && !(2 in uncertified)
    @test ok[2] == eval_tree_array(plain, X, ops)[2]
    @test ok[1] && !eval_tree_array(quirk, X, ops)[2]      # the documented divergence, and why tree 1 is listed
    # (b) forward duals are the default of the fused loss gradient; reverse_grad=true is the permission for reverse accumulation: same
    #     values to rounding
    wide = sum(Node{Float64}(; val=0.1 * k) * Node{Float64}(; feature=1 + k % 2) for k in 1:10)   # 10 constants: reverse where allowed
    X64 = randn(Float64, 2, 2_000); y = randn(Float64, 2_000)
    ops64 = OperatorEnum(1 => (cos, exp), 2 => (+, -, /, *))
    pf = HIP.HIPPopulation([wide], ops64, 2)
    pr = HIP.HIPPopulation([wide], ops64, 2; reverse_grad=true)
    lf, df, okf = HIP.eval_population_loss_grad(pf, X64, y)
    lr, dr, okr = HIP.eval_population_loss_grad(pr, X64, y)
    @test okf == okr && isapprox(lf, lr; rtol=1e-12) && isapprox(df[1], dr[1]; rtol=1e-9)
    # (c) trim_context! frees what the task's context retains; the next population simply allocates afresh
    HIP.trim_context!()
    out2, ok2 = HIP.eval_population(HIP.HIPPopulation([plain], ops, 2), X)
    @test ok2[1] == ok[2] && agree(view(out2, :, 1), view(out, :, 2))
end

@testset "minibatches: the row sampler against its definition, the gather against indexing (DESIGN.md §4.4.18)" begin
    # the definition of include/de_hip.h restated: wrapping UInt64 arithmetic is Julia's own
    G = 0x9E3779B97F4A7C15
    fin(z::UInt64) = (z ⊻= z >> 30; z *= 0xBF58476D1CE4E5B9; z ⊻= z >> 27; z *= 0x94D049BB133111EB; z ⊻ (z >> 31))
    key(seed, step) = fin(UInt64(seed) ⊻ fin(UInt64(step) + G))
    replace_row(k, N, i) = Int64((UInt128(fin(k + G * UInt64(i + 1))) * UInt128(N)) >> 64) + 1
    @test fin(G) == 0xe220a8397b1dcdaf && key(1, 0) == 0x9e0160293a33aaf7
    ops = OperatorEnum(1 => (cos, exp), 2 => (+, -, /, *))
    x1, x2 = Node{Float32}(; feature=1), Node{Float32}(; feature=2)
    pop = HIP.HIPPopulation([x1 * cos(x2 - 3.2f0), x1 + x2 * 0.5f0], ops, 2)
    N = 5_000
    rows = HIP.sample_population_rows(pop, N, 1_000; seed=1, step=3)
    @test rows == [replace_row(key(1, 3), N, j) for j in 0:999]
    @test HIP.sample_population_rows(pop, 10, 8; seed=1) == [5, 2, 9, 1, 3, 2, 1, 2] .+ 1
    @test HIP.sample_population_rows(pop, 10, 3; seed=1, offset=5) == [2, 1, 2] .+ 1      # a batch drawn in pieces
    perm = HIP.sample_population_rows(pop, 10, 10; seed=5, step=2, mode=:permute)
    @test perm == [9, 7, 0, 1, 2, 3, 6, 8, 4, 5] .+ 1 && sort(perm) == collect(1:10)
    @test_throws Exception HIP.sample_population_rows(pop, 10, 11; seed=5, mode=:permute)
    X = randn(Float32, 2, N); y = randn(Float32, N); w = rand(Float32, N)
    b = HIP.gather_population_batch(pop, X, rows; y=y, weights=w)
    @test b.X == X[:, rows] && b.y == y[rows] && b.weights == w[rows] && b.classes === nothing
    @test_throws Exception HIP.gather_population_batch(pop, X, [1, N + 1]; y=y)
    # the batch is a dataset like any other: the same bits as the same rows gathered by indexing
    l1, ok1 = HIP.eval_population_loss(pop, b.X, b.y; weights=b.weights)
    l2, ok2 = HIP.eval_population_loss(pop, X[:, rows], y[rows]; weights=w[rows])
    l3, ok3, b3 = HIP.eval_population_loss_minibatch(pop, X, y, 1_000; seed=1, step=3, weights=w)
    @test ok1 == ok2 == ok3 && l1 == l2 == l3 && b3.rows == rows
end
