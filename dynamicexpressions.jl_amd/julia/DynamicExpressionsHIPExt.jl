# DynamicExpressionsHIPExt.jl — the reference-side binding of libde_hip.so.
#
# This is the Julia half of the boundary (SURVEY.md §8b, INTEGRATION.md): it stays entirely on
# the host, keeps the reference's Node / OperatorEnum / EvalContext API, flattens a tree into
# the post-order tape of include/de_hip.h and `ccall`s the C ABI.  It mirrors, line for line,
# what the Python twin (dynamicexpressions.jl_amd/node.py + api.py) does; the Python twin is the
# one exercised by the test-suite because the build image has no Julia.
#
# Plug-in point: exactly the precedent of the Bumper whole-tree override
#   ext/DynamicExpressionsBumperExt.jl:11-49   _bumper_eval_tree_array(tree, cX, operators, ctx)
#   src/ExtensionInterface.jl:60-64            bumper_eval_tree_array stub
#   src/Evaluate.jl:300-302                    `if bumper isa Val{true} return bumper_eval_tree_array(...)`
# A maintainer adds the analogous stub `hip_eval_tree_array` (INTEGRATION.md §3) and this file
# as a package extension keyed on a weak dependency that provides the shared library.
module DynamicExpressionsHIPExt

using DynamicExpressions:
    AbstractExpressionNode, Node, GraphNode, OperatorEnum, EvalContext, get_child, get_children,
    count_constant_nodes, preserve_sharing, ParametricExpression, get_contents, get_metadata
import DynamicExpressions.ExtensionInterfaceModule: is_extension_loaded

const LIBDE = get(ENV, "DE_HIP_LIB", "libde_hip")

# ---- de_hip.h mirrors ---------------------------------------------------------------------
struct TapeNode            # de_tape_node_t
    degree::UInt8
    op::UInt8
    arg::UInt16
end
const DE_OK = Cint(0)
const DE_ERR_UNSUPPORTED_OP = Cint(3)
const DE_LEAF_CONST, DE_LEAF_FEATURE, DE_LEAF_PARAM, DE_LEAF_SHARED = UInt8(0), UInt8(1), UInt8(2), UInt8(3)
const DE_OP_SHARE = UInt8(0xFE)   # include/de_opcodes.h: "the subtree just emitted is shared subtree `arg`"
const DE_F32, DE_F64, DE_F16, DE_CF32, DE_CF64 = Cint(0), Cint(1), Cint(2), Cint(3), Cint(4)
const DE_OPT_EARLY_EXIT, DE_OPT_FUSE_DEG1, DE_OPT_FUSE_DEG2, DE_OPT_BUMPER_CHECKS, DE_OPT_TURBO, DE_OPT_FULL_EVAL, DE_OPT_FORWARD_GRAD, DE_OPT_REVERSE_GRAD =
    UInt32(1), UInt32(2), UInt32(4), UInt32(8), UInt32(16), UInt32(32), UInt32(64), UInt32(128)
const DE_OPT_F16_GRAD = UInt32(256)   # a Float16 program with it serves de_eval_grad / de_eval_diff (DESIGN.md §13.6)
const DE_OPT_TYPED_LOSS = UInt32(512) # a Float16 / complex program with it serves de_eval_loss(_ex), L2 and L1 (DESIGN.md §4.4.17)
# The ABI this file was written for (include/de_hip.h lists what changed between versions).  Version 2: the rows / gradients of a tree
# with `complete == false` are NOT evaluated to the end (the reference's early exit, src/Evaluate.jl:26-32): with the host arrays this
# shim passes, the library NaN-fills them; `full_eval=true` (DE_OPT_FULL_EVAL) evaluates every tree on every sample instead.
# Version 3: fused loss gradients run forward duals (the reference's flag semantics) unless `reverse_grad=true` (DE_OPT_REVERSE_GRAD).
const DE_HIP_ABI_VERSION = Cint(3)
function __init__()
    v = try
        ccall((:de_abi_version, LIBDE), Cint, ())
    catch
        return nothing   # library not present: every entry point fails loudly when it is used
    end
    v == DE_HIP_ABI_VERSION || error("libde_hip has ABI version $(v), DynamicExpressionsHIPExt was written for $(DE_HIP_ABI_VERSION)")
    return nothing
end
const OPERATOR_LIMIT_BEFORE_SLOWDOWN = 15   # src/Evaluate.jl:14
dtype_code(::Type{Float32}) = DE_F32
dtype_code(::Type{Float64}) = DE_F64
# Float16: every operator step rounded to binary16 (DESIGN.md §13).  eval_grad_tree_array / eval_diff_tree_array create their program
# with DE_OPT_F16_GRAD (binary16 duals, DESIGN.md §13.6); losses, pullbacks and fits stay Float32 / Float64 and keep the reference CPU path
dtype_code(::Type{Float16}) = DE_F16
# ComplexF32 / ComplexF64: evaluation only (Julia's Complex methods of 19 opcodes, DESIGN.md §14); a tree with another operator and every
# complex gradient keep the reference CPU path
dtype_code(::Type{ComplexF32}) = DE_CF32
dtype_code(::Type{ComplexF64}) = DE_CF64

struct UnsupportedOperator <: Exception
    f::Any
    degree::Int
end

# ---- OperatorEnum -> opcode table: by function IDENTITY ----------------------------------------
# An OperatorEnum holds arbitrary Julia functions (src/OperatorEnum.jl:14-49); the device knows a closed set of
# opcodes (include/de_opcodes.h).  A function is mapped onto an opcode only when it IS one of the functions below
# (`===`): Base's own `cos`, `+`, `max` ... .  A user function that merely shares a name with one of them (`cos(x) =
# my_cos(x)`, an anonymous function, a method-extended copy in another module) is NOT the same object and has no opcode:
# `opcode_table` throws `UnsupportedOperator` and the caller keeps the reference CPU path — never wrong values with
# `complete = true`.
const BASE_OPCODES = let t = IdDict{Any,Tuple{Vararg{Pair{Int,String}}}}()
    reg(f, pairs...) = (t[f] = pairs)
    for (f, n) in ((sin, "sin"), (cos, "cos"), (tan, "tan"), (exp, "exp"), (exp2, "exp2"), (log, "log"), (log2, "log2"),
                   (log10, "log10"), (log1p, "log1p"), (sqrt, "sqrt"), (cbrt, "cbrt"), (abs, "abs"), (sinh, "sinh"),
                   (cosh, "cosh"), (tanh, "tanh"), (asin, "asin"), (acos, "acos"), (atan, "atan"), (asinh, "asinh"),
                   (acosh, "acosh"), (atanh, "atanh"), (round, "round"), (floor, "floor"), (ceil, "ceil"), (sign, "sign"),
                   (inv, "inv"), (abs2, "square"))
        reg(f, 1 => n)
    end
    reg(-, 1 => "neg", 2 => "-")                       # unary minus and subtraction are the same Julia function
    reg(+, 2 => "+", 3 => "+")
    reg(max, 2 => "max", 3 => "max")
    for (f, n) in ((*, "*"), (/, "/"), (^, "^"), (min, "min"), (mod, "mod"), (rem, "rem"))
        reg(f, 2 => n)
    end
    reg(fma, 3 => "fma")
    reg(clamp, 3 => "clamp")
    t
end
# Functions that are NOT in Base — the helpers the reference's own tests define (`safe_log`, `relu`, `square`, `cube`,
# `custom_cos`, `pow_abs2`, `greater`, `sub` ..., test/test_params.jl:7-29) or SpecialFunctions.gamma — have opcodes too,
# but only the user can vouch that THEIR function of that name has those semantics (and that gradient):
#     register_hip_opcode(my_safe_log, :safe_log)
# The registration probes the function on a few points against the opcode's definition and refuses a mismatch.
const USER_OPCODES = IdDict{Any,Tuple{Int,String}}()
const USER_OPCODES_LOCK = ReentrantLock()
const PROBES = (0.37, 1.0, 2.5, -0.6, -2.25)
const OPCODE_SEMANTICS = Dict{Symbol,Function}(
    :safe_log => x -> x > 0 ? log(x) : NaN, :safe_log2 => x -> x > 0 ? log2(x) : NaN, :safe_log10 => x -> x > 0 ? log10(x) : NaN,
    :safe_log1p => x -> x > -1 ? log1p(x) : NaN, :safe_sqrt => x -> x >= 0 ? sqrt(x) : NaN, :safe_acosh => x -> x >= 1 ? acosh(x) : NaN,
    :relu => x -> x < 0 ? zero(x) : x, :square => x -> x * x, :cube => x -> x * x * x, :neg => x -> -x, :custom_cos => x -> cos(x)^2,
    :greater => (x, y) -> x > y ? 1.0 : 0.0, :sub => (x, y) -> x - y, :pow_abs2 => (x, y) -> exp(y * log(abs(x))),
    :add => (x, y) -> x + y, :mult => (x, y) -> x * y, :div => (x, y) -> x / y, :pow => (x, y) -> x^y,
)
"""
    register_hip_opcode(f, name::Symbol)

Declare that the user function `f` computes the device operator `name` (one of `keys(OPCODE_SEMANTICS)`, or `:gamma`).
`f` is probed against the operator's definition on a few points (NaN pattern included); a mismatch throws.  Registration
is by identity: other functions of the same name stay on the CPU path.
"""
function register_hip_opcode(f, name::Symbol)
    degree = first(methods(f)).nargs - 1
    code = ccall((:de_opcode_by_name, LIBDE), Cint, (Cstring, Cint), String(name), degree)
    code < 0 && throw(ArgumentError("no device operator $(name) of degree $(degree)"))
    if haskey(OPCODE_SEMANTICS, name)
        g = OPCODE_SEMANTICS[name]
        for x in PROBES, y in (degree == 2 ? PROBES : (0.0,))
            a = try degree == 1 ? f(x) : f(x, y) catch; NaN end     # DomainError == NaN on the device
            b = degree == 1 ? g(x) : g(x, y)
            (isnan(a) && isnan(b)) || isapprox(a, b; rtol=1e-12) ||
                throw(ArgumentError("$(f) is not the operator $(name): f($(x)$(degree == 2 ? ", $(y)" : "")) = $(a), expected $(b)"))
        end
    end
    lock(USER_OPCODES_LOCK) do
        USER_OPCODES[f] = (degree, String(name))
    end
    return f
end

function opcode_of(f, d::Int)
    name = nothing
    if haskey(BASE_OPCODES, f)
        for (deg, n) in BASE_OPCODES[f]
            deg == d && (name = n)
        end
    else
        entry = lock(() -> get(USER_OPCODES, f, nothing), USER_OPCODES_LOCK)
        entry !== nothing && entry[1] == d && (name = entry[2])
    end
    name === nothing && throw(UnsupportedOperator(f, d))
    code = ccall((:de_opcode_by_name, LIBDE), Cint, (Cstring, Cint), name, d)
    code < 0 && throw(UnsupportedOperator(f, d))
    return UInt8(code)
end

"""Opcode of every operator of `operators`, per degree; throws `UnsupportedOperator` for a
function that is neither one of Base's (by identity) nor registered (the caller then keeps the CPU path)."""
function opcode_table(operators::OperatorEnum)
    return ntuple(d -> map(f -> opcode_of(f, d), operators.ops[d]), length(operators.ops))
end

"""EvalContext knobs that change RESULTS -> de_options bits (src/Evaluate.jl:156-181,496,607)."""
function option_bits(operators::OperatorEnum, ctx::EvalContext; full_eval::Bool=false, forward_grad::Bool=false, reverse_grad::Bool=false, half_grad::Bool=false, typed_loss::Bool=false)
    nops(d) = d <= length(operators.ops) ? length(operators.ops[d]) : 0
    fused = ctx.use_fused isa Val{true}
    bits = UInt32(0)
    ctx.early_exit isa Val{true} && (bits |= DE_OPT_EARLY_EXIT)
    fused && nops(1) <= OPERATOR_LIMIT_BEFORE_SLOWDOWN && (bits |= DE_OPT_FUSE_DEG1)
    fused && nops(2) <= OPERATOR_LIMIT_BEFORE_SLOWDOWN && (bits |= DE_OPT_FUSE_DEG2)
    ctx.bumper isa Val{true} && (bits |= DE_OPT_BUMPER_CHECKS)
    ctx.turbo isa Val{true} && (bits |= DE_OPT_TURBO)   # the LoopVectorization knob = the relaxed-accuracy device operators
    full_eval && (bits |= DE_OPT_FULL_EVAL)             # no early exit at tree granularity: rows of incomplete trees are fully evaluated
    forward_grad && (bits |= DE_OPT_FORWARD_GRAD)       # ABI 2's spelling of what is the default since ABI 3: fused loss gradients by forward duals (the reference's flag semantics exactly)
    half_grad && (bits |= DE_OPT_F16_GRAD)              # Float16 programs: de_eval_grad / de_eval_diff in binary16 steps (other element types ignore it)
    typed_loss && (bits |= DE_OPT_TYPED_LOSS)           # Float16 / complex programs: de_eval_loss(_ex) for L2 and L1 (Float32 / Float64 ignore it)
    reverse_grad && (bits |= DE_OPT_REVERSE_GRAD)       # permission for reverse accumulation (faster from 8 gradient rows per tree on; `ok` may differ in ~0.03 % of Float32 cases)
    return bits
end

# ---- flattening: post-order tape + constant pool (depth-first, left to right) ---------------
# (`cbase` = length(consts) when the tree starts: constant slots are numbered per tree, the pool of a population is shared)
function flatten!(
    nodes::Vector{TapeNode}, consts::Vector{T}, tree::AbstractExpressionNode{T}, optable, cbase::Int=0
) where {T}
    if tree.degree == 0
        if tree.constant
            push!(consts, tree.val)
            push!(nodes, TapeNode(0x00, DE_LEAF_CONST, UInt16(length(consts) - 1 - cbase)))
        elseif hasproperty(tree, :is_parameter) && tree.is_parameter   # ParametricNode
            push!(nodes, TapeNode(0x00, DE_LEAF_PARAM, UInt16(tree.parameter - 1)))
        else
            push!(nodes, TapeNode(0x00, DE_LEAF_FEATURE, UInt16(tree.feature - 1)))
        end
    else
        d = Int(tree.degree)
        for c in get_children(tree, d)
            flatten!(nodes, consts, c, optable, cbase)
        end
        push!(nodes, TapeNode(UInt8(d), optable[d][tree.op], 0x0000))
    end
    return nothing
end

# ---- GraphNode (src/Node.jl:138-166): the CSE tape of de_program_create_cse -------------------------------------
# `flatten!` above walks a GraphNode like the reference's evaluator does — a shared node once per parent — and gives the
# EXPANDED tape with one constant slot per occurrence.  `flatten_cse!` restates the tree with every shared, non-constant
# operator subtree once: DE_OP_SHARE after its first occurrence, DE_LEAF_SHARED afterwards; constant leaves keep the slot
# of their first occurrence in the expanded numbering.  Returns the number of shared subtrees (0: pass an empty range).
# `occurrence_map` gives, per expanded slot, the index of the unique constant (get_scalar_constants order): the shim keeps
# occurrence slots equal (set_population_constants!) and sums their gradient rows.
function flatten_cse!(nodes::Vector{TapeNode}, tree::AbstractExpressionNode{T}, optable) where {T}
    isconst = IdDict{Any,Bool}()
    nparents = IdDict{Any,Int}()
    # every node OBJECT once: nparents[c] = the number of (parent object, child slot) pairs that hold c — more than one
    # distinct parent, or the same parent twice, is what makes a subtree shared in its own right (a node reached only
    # through an already-shared ancestor has one).  Mirrors `multi_use` of the Python twin (node.py flatten_graph).
    function survey(n)
        haskey(isconst, n) && return nothing
        if n.degree == 0
            isconst[n] = n.constant
        else
            cs = get_children(n, Int(n.degree))
            for c in cs
                nparents[c] = get(nparents, c, 0) + 1
                survey(c)
            end
            isconst[n] = all(c -> isconst[c], cs)
        end
        return nothing
    end
    survey(tree)
    defined = IdDict{Any,Int}()
    slot = Ref(0)
    skip(n) = n.degree == 0 ? (n.constant && (slot[] += 1)) : foreach(skip, get_children(n, Int(n.degree)))
    function emit(n, under_ternary::Bool)
        if haskey(defined, n)
            push!(nodes, TapeNode(0x00, DE_LEAF_SHARED, UInt16(defined[n])))
            skip(n)
            return
        end
        if n.degree == 0
            if n.constant
                push!(nodes, TapeNode(0x00, DE_LEAF_CONST, UInt16(slot[]))); slot[] += 1
            else
                push!(nodes, TapeNode(0x00, DE_LEAF_FEATURE, UInt16(n.feature - 1)))
            end
            return
        end
        d = Int(n.degree)
        foreach(c -> emit(c, d == 3), get_children(n, d))
        push!(nodes, TapeNode(UInt8(d), optable[d][n.op], 0x0000))
        if get(nparents, n, 0) > 1 && !isconst[n] && !under_ternary && n !== tree && length(defined) < 12
            defined[n] = length(defined)
            push!(nodes, TapeNode(0x01, DE_OP_SHARE, UInt16(defined[n])))
        end
    end
    emit(tree, false)
    return length(defined)
end
function occurrence_map(tree::AbstractExpressionNode)
    uniq = IdDict{Any,Int}()
    occ = Int[]
    walk(n) = n.degree == 0 ? (n.constant && push!(occ, get!(uniq, n, length(uniq) + 1))) : foreach(walk, get_children(n, Int(n.degree)))
    walk(tree)
    return occ
end

# ---- context: one de_ctx_t per Julia TASK ---------------------------------------------------
# A de_ctx_t is not thread-safe (INTEGRATION.md §4): every call on it — and the destruction of programs that live in it,
# which finalizers run from arbitrary threads — takes the context's lock.  Programs hold a strong reference to their
# context, so a context is finalized only after all of its programs; destroying a program whose context is already gone
# (process exit, finalizer order unspecified) is a no-op.
mutable struct HIPContext
    handle::Ptr{Cvoid}
    lock::ReentrantLock
end
# Finalizers must not block on a lock a running task may hold: when the lock is taken, the SAME cleanup is registered again
# (the object survives this collection and the next one retries) — re-arming with `identity` would leak the handle.
function finalize_context(c::HIPContext)
    if trylock(c.lock)
        try
            c.handle != C_NULL && ccall((:de_ctx_destroy, LIBDE), Cint, (Ptr{Cvoid},), c.handle)
            c.handle = C_NULL
        finally
            unlock(c.lock)
        end
    else
        finalizer(finalize_context, c)
    end
    return nothing
end
# (Several contexts on DIFFERENT devices may live in one process: the library caches its handler tables per device, ABI version 2.)
function HIPContext(device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:de_ctx_create, LIBDE), Cint, (Cint, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), device, C_NULL, h)
    rc == DE_OK || error("de_ctx_create failed: ", unsafe_string(ccall((:de_status_string, LIBDE), Cstring, (Cint,), rc)))
    ctx = HIPContext(h[], ReentrantLock())
    finalizer(finalize_context, ctx)
    return ctx
end
"""The calling task's context (task-local storage: tasks migrate between threads, `Threads.threadid()` is not a key)."""
task_context() = get!(() -> HIPContext(0), task_local_storage(), :DynamicExpressionsHIPExt_context)::HIPContext
"""Free what the context retains between populations (the parked host vectors and recycled device buffers of destroyed populations —
up to 512 MB of host and 256 MB of device memory per context, i.e. per task — and the staging scratch of host arrays): `de_ctx_trim`.
Call it from a task that goes idle; the next population simply allocates afresh."""
function trim_context!(ctx::HIPContext=task_context())
    with_ctx(ctx) do h
        check(ctx, ccall((:de_ctx_trim, LIBDE), Cint, (Ptr{Cvoid},), h))
    end
    return nothing
end

function check(ctx::HIPContext, rc::Cint)
    rc == DE_OK && return true
    rc == DE_ERR_UNSUPPORTED_OP && throw(UnsupportedOperator(nothing, 0))
    error(unsafe_string(ccall((:de_last_error, LIBDE), Cstring, (Ptr{Cvoid},), ctx.handle)))
end
"""Run `f(handle)` holding the context's lock."""
with_ctx(f, ctx::HIPContext) = lock(() -> (ctx.handle == C_NULL && error("HIP context was destroyed"); f(ctx.handle)), ctx.lock)

# ---- the whole-tree override (signature of _bumper_eval_tree_array) --------------------------
"""
    _hip_eval_tree_array(tree, cX, operators, eval_context) -> (result::Vector{T}, ok::Bool)

Drop-in for `eval_tree_array`'s body: same `(output, complete)` tuple, `cX` is the reference's
`[n_features, n_rows]` column-major matrix and is passed zero-copy.  Falls back to the CPU path
(returns `nothing`) when an operator has no device opcode.
"""
function _hip_eval_tree_array(
    tree::AbstractExpressionNode{T}, cX::AbstractMatrix{T}, operators::OperatorEnum,
    eval_context::EvalContext; full_eval::Bool=false,
) where {T<:Union{Float16,Float32,Float64,ComplexF32,ComplexF64}}
    optable = try
        opcode_table(operators)
    catch e
        e isa UnsupportedOperator || rethrow()
        return nothing                       # caller continues on the reference CPU path
    end
    nodes, consts = TapeNode[], T[]
    flatten!(nodes, consts, tree, optable)
    F, N = size(cX)
    X = cX isa Matrix{T} ? cX : Matrix{T}(cX)  # strided views are copied; Matrix is zero-copy
    out = Vector{T}(undef, N)
    ok = Ref{UInt8}(0)
    ctx = task_context()
    rc = with_ctx(ctx) do h
        GC.@preserve nodes consts X out ccall(
            (:de_eval_tree_array, LIBDE), Cint,
            (Ptr{Cvoid}, Cint, Ptr{TapeNode}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int32, Int64, UInt32,
             Ptr{Cvoid}, Ref{UInt8}),
            h, dtype_code(T), nodes, length(nodes), consts, length(consts), X, F, N,
            option_bits(operators, eval_context; full_eval), out, ok)
    end
    # a complex tree with an operator that has no complex kernel (abs, max, ...): the reference CPU path
    T <: Complex && rc == DE_ERR_UNSUPPORTED_OP && return nothing
    check(ctx, rc)
    return (out, ok[] != 0x00)   # ok == false: `out` is all NaN unless full_eval (only the flag is contractual, SURVEY.md §8a)
end

# ---- population form: lower many trees once, evaluate in one launch -------------------------
# GraphNode populations: the library keeps one constant slot per OCCURRENCE of a constant leaf (the expanded tape); to the user a
# shared constant is ONE constant (count_constant_nodes with f_on_shared, src/NodeUtils.jl:43-51) with ONE gradient row (the shared
# NodeIndex entry, :184-201).  `occ[t]` (occurrence_map) maps tree t's slots to its unique constants — `nothing` when no constant
# of the tree is shared —, `n_slots[t]` / `n_consts[t]` count both: set_population_constants! fans values out, the gradient
# entry points sum the occurrence rows (combine_rows) — the mirror of api.py's `_occ` / `_combine_rows`.
mutable struct HIPPopulation{T}
    ctx::HIPContext
    handle::Ptr{Cvoid}
    n_trees::Int
    n_features::Int
    occ::Vector{Union{Nothing,Vector{Int}}}
    n_slots::Vector{Int}
    n_consts::Vector{Int}
    optable::Any                                  # opcode_table of the population's operators (update_population! flattens with it)
end
function finalize_population(p::HIPPopulation)
    c = p.ctx
    if trylock(c.lock)
        try
            # de_program_destroy synchronises the context's stream: skip it when the context is already gone
            c.handle != C_NULL && p.handle != C_NULL && ccall((:de_program_destroy, LIBDE), Cint, (Ptr{Cvoid},), p.handle)
            p.handle = C_NULL
        finally
            unlock(c.lock)
        end
    else
        finalizer(finalize_population, p)   # lock taken: the same cleanup again at the next collection (see finalize_context)
    end
    return nothing
end
"""Run `f(context handle, program handle)` holding the lock of the population's context (every entry point does: a `de_ctx_t` is
not thread-safe, and `finalize_population` of ANOTHER population of the same context may run on a GC thread at any time)."""
function with_pop(f, pop::HIPPopulation)
    return with_ctx(pop.ctx) do h
        pop.handle == C_NULL && error("HIP population was destroyed")
        f(h, pop.handle)
    end
end
function HIPPopulation(
    trees::AbstractVector{<:AbstractExpressionNode{T}}, operators::OperatorEnum, n_features::Integer;
    eval_context::EvalContext=EvalContext(), n_params::Integer=0, full_eval::Bool=false, forward_grad::Bool=false,
    reverse_grad::Bool=false, half_grad::Bool=false, typed_loss::Bool=false,
) where {T<:Union{Float16,Float32,Float64,ComplexF32,ComplexF64}}
    optable = opcode_table(operators)
    nodes, consts, cse = TapeNode[], T[], TapeNode[]
    node_off, const_off, cse_off = Int64[0], Int64[0], Int64[0]
    occ = Union{Nothing,Vector{Int}}[]
    n_slots, n_consts = Int[], Int[]
    for t in trees
        c0 = length(consts)
        flatten!(nodes, consts, t, optable, c0)   # constant slots are numbered PER TREE (de_tape_node_t.arg)
        push!(node_off, length(nodes)); push!(const_off, length(consts))
        o = nothing
        if preserve_sharing(typeof(t))            # GraphNode: a second, CSE tape for the eval program
            mark = length(cse)
            flatten_cse!(cse, t, optable) == 0 && resize!(cse, mark)
            om = occurrence_map(t)
            (!isempty(om) && maximum(om) < length(om)) && (o = om)   # some constant leaf occurs more than once
        end
        push!(cse_off, length(cse))
        push!(occ, o)
        push!(n_slots, length(consts) - c0)
        push!(n_consts, o === nothing ? length(consts) - c0 : maximum(o))
    end
    ctx = task_context()
    h = Ref{Ptr{Cvoid}}(C_NULL)
    with_ctx(ctx) do hc
        check(ctx, GC.@preserve nodes consts node_off const_off cse cse_off ccall(
            (:de_program_create_cse, LIBDE), Cint,
            (Ptr{Cvoid}, Cint, Ptr{TapeNode}, Ptr{Int64}, Ptr{TapeNode}, Ptr{Int64}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int32, Int32,
             UInt32, Ref{Ptr{Cvoid}}),
            hc, dtype_code(T), nodes, node_off, isempty(cse) ? C_NULL : pointer(cse), cse_off, length(trees), consts,
            const_off, n_features, n_params, option_bits(operators, eval_context; full_eval, forward_grad, reverse_grad, half_grad, typed_loss), h))
    end
    pop = HIPPopulation{T}(ctx, h[], length(trees), n_features, occ, n_slots, n_consts, optable)
    finalizer(finalize_population, pop)
    return pop
end
"""
    update_population!(pop, ids, trees)

Replace trees `ids` (1-based) of `pop` by `trees` in place (`de_program_update`, DESIGN.md §3.4): flattened as `HIPPopulation` does,
the result is what a fresh `HIPPopulation` of the resulting trees would be.  A captured graph of the population must be re-captured.
"""
function update_population!(
    pop::HIPPopulation{T}, ids::AbstractVector{<:Integer}, trees::AbstractVector{<:AbstractExpressionNode{T}},
) where {T}
    length(ids) == length(trees) || throw(ArgumentError("update_population!: $(length(ids)) ids for $(length(trees)) trees"))
    allunique(ids) || throw(ArgumentError("update_population!: a tree id appears twice"))
    all(t -> 1 <= t <= pop.n_trees, ids) || throw(ArgumentError("update_population!: tree id outside 1:$(pop.n_trees)"))
    isempty(ids) && return pop
    optable = pop.optable
    nodes, consts, cse = TapeNode[], T[], TapeNode[]
    node_off, const_off, cse_off = Int64[0], Int64[0], Int64[0]
    occ = Union{Nothing,Vector{Int}}[]
    n_slots, n_consts = Int[], Int[]
    for t in trees
        c0 = length(consts)
        flatten!(nodes, consts, t, optable, c0)
        push!(node_off, length(nodes)); push!(const_off, length(consts))
        o = nothing
        if preserve_sharing(typeof(t))
            mark = length(cse)
            flatten_cse!(cse, t, optable) == 0 && resize!(cse, mark)
            om = occurrence_map(t)
            (!isempty(om) && maximum(om) < length(om)) && (o = om)
        end
        push!(cse_off, length(cse))
        push!(occ, o)
        push!(n_slots, length(consts) - c0)
        push!(n_consts, o === nothing ? length(consts) - c0 : maximum(o))
    end
    ids0 = Int64[t - 1 for t in ids]
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve ids0 nodes consts node_off const_off cse cse_off ccall(
            (:de_program_update, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{TapeNode}, Ptr{Int64}, Ptr{TapeNode}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}),
            hp, ids0, length(ids0), nodes, node_off, isempty(cse) ? C_NULL : pointer(cse), isempty(cse) ? C_NULL : pointer(cse_off),
            isempty(consts) ? C_NULL : pointer(consts), const_off))
    end
    for (i, t) in enumerate(ids)
        pop.occ[t] = occ[i]
        pop.n_slots[t] = n_slots[i]
        pop.n_consts[t] = n_consts[i]
    end
    return pop
end
"""Gradient rows (or entries) of tree `t` in the library's per-occurrence layout -> the reference's layout: the rows of a shared
constant are summed.  `g` is a vector of entries or a matrix with one ROW per gradient component; the `lead` rows in front of
the constants (features in `:both` mode) pass through.  `mode == 0` (`variable=true`) has no constant rows."""
function combine_rows(pop::HIPPopulation, t::Integer, g::AbstractVecOrMat, mode::Integer)
    o = pop.occ[t]
    (o === nothing || mode == 0) && return g
    lead = size(g, 1) - length(o)
    nu = pop.n_consts[t]
    out = g isa AbstractVector ? zeros(eltype(g), lead + nu) : zeros(eltype(g), lead + nu, size(g, 2))
    if g isa AbstractVector
        out[1:lead] .= g[1:lead]
        for (k, u) in enumerate(o)
            out[lead + u] += g[lead + k]
        end
    else
        out[1:lead, :] .= g[1:lead, :]
        for (k, u) in enumerate(o)
            out[lead + u, :] .+= g[lead + k, :]
        end
    end
    return out
end

"""`(out::Matrix{T}(N × n_trees), ok::Vector{Bool})`; column t is `eval_tree_array(trees[t], X)`.  Columns with `ok[t] == false`
are NaN (the tree left the kernel at its first flagged workgroup, like the reference's early return) unless the population
was made with `full_eval=true`."""
function eval_population(pop::HIPPopulation{T}, X::Matrix{T}) where {T}
    F, N = size(X)
    @assert F >= pop.n_features
    out = Matrix{T}(undef, N, pop.n_trees)          # row t of the C layout = column t here
    ok = Vector{UInt8}(undef, pop.n_trees)
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X out ok ccall(
            (:de_eval, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{UInt8}),
            hc, hp, X, N, F, C_NULL, out, N, ok))
    end
    return out, ok .!= 0x00
end

"""
    population_sum_certificate(pop, X) -> (ok, certified, max_abs)

`de_eval_sum_certificate`: the reference tests `isfinite(sum(x))` (src/ValueInterface.jl:9), the kernels every element; `certified[t]`
says the two provably agree for tree t (some element non-finite, or `N * max|tested value|` below `floatmax(T)`).  Only the trees
with `certified[t] == false` can carry a flag that differs from `eval_tree_array`'s — re-derive those on the CPU when the bit matters.
"""
function population_sum_certificate(pop::HIPPopulation{T}, X::Matrix{T}) where {T}
    F, N = size(X)
    @assert F >= pop.n_features
    ok = Vector{UInt8}(undef, pop.n_trees)
    cert = Vector{UInt8}(undef, pop.n_trees)
    mx = Vector{Float64}(undef, pop.n_trees)
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X ok cert mx ccall(
            (:de_eval_sum_certificate, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}),
            hc, hp, X, N, F, C_NULL, ok, cert, mx))
    end
    return ok .!= 0x00, cert .!= 0x00, mx
end

"""
    eval_population_strict(pop, X) -> (out, ok, uncertified::Vector{Int})

`eval_population` followed by the certificate pass: `uncertified` lists (1-based) the trees whose element-wise flag is NOT provably the
reference's `isfinite(sum(x))` flag — for every other tree `ok[t]` IS `eval_tree_array`'s `complete`.  A caller who needs the
reference's bit re-derives only those trees on the CPU (`strict_flags` of the Python twin).
"""
function eval_population_strict(pop::HIPPopulation{T}, X::Matrix{T}) where {T}
    out, ok = eval_population(pop, X)
    ok2, cert, _ = population_sum_certificate(pop, X)
    ok2 == ok || error("strict flags: the certificate pass and the evaluation disagree on a flag")
    return out, ok, findall(!, cert)
end

struct ParamArgs            # de_param_args_t
    params::Ptr{Cvoid}
    ld_params::Int64
    n_classes::Int64
    classes::Ptr{Cvoid}
    classes_is_i64::Int32
    class_base::Int32
end

"""
    eval_population(pop, X, parameters, classes) -> (out, ok)

ParametricExpression form (src/ParametricExpression.jl:371-390): `parameters` is the `P × C` matrix,
`classes::Vector{Int}` the 1-based class of every column of `X`; the `P × N` gather the reference
materialises is done on the fly in the kernel.  The range assertions of the reference (:378-379) are
repeated here because the library trusts the ids.
"""
function eval_population(
    pop::HIPPopulation{T}, X::Matrix{T}, parameters::Matrix{T}, classes::Vector{Int}
) where {T}
    F, N = size(X)
    @assert length(classes) == N
    @assert isempty(classes) || (minimum(classes) >= 1 && maximum(classes) <= size(parameters, 2))
    out = Matrix{T}(undef, N, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X parameters classes out ok begin
            pa = Ref(ParamArgs(pointer(parameters), size(parameters, 1), size(parameters, 2), pointer(classes), 1, 1))
            ccall((:de_eval, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{ParamArgs}, Ptr{Cvoid}, Int64, Ptr{UInt8}),
                hc, hp, X, N, F, pa, out, N, ok)
        end)
    end
    return out, ok .!= 0x00
end

struct LossSpec             # de_loss_spec_t
    kind::Int32
    reserved::Int32
    param::Float64
end
# de_loss_kind_t (include/de_hip.h has the formulas): e = ŷ - y, a = y * ŷ for the two margin kinds
const LOSS_KINDS = Dict{Symbol,Int32}(
    :L2 => 0, :L1 => 1, :pullback => 2, :huber => 16, :logcosh => 17, :l1_eps => 18, :l2_eps => 19, :quantile => 20, :lp => 21,
    :logit_dist => 22, :logit_margin => 23, :l1_hinge => 24,
)
"""The `de_loss_spec_t` of a loss name and its parameter (`:pullback` belongs to the gradient entry points).  The library checks the
parameter's range (`de_loss_spec_check`) inside the call and answers `DE_ERR_INVALID_ARG`, naming the kind, before it touches an output."""
function loss_spec(loss::Symbol, loss_param::Real; with_gradient::Bool=true)
    (haskey(LOSS_KINDS, loss) && (with_gradient || loss !== :pullback)) || throw(ArgumentError("unknown loss $loss"))
    return Ref(LossSpec(LOSS_KINDS[loss], Int32(0), Float64(loss_param)))
end

# element types of a fused loss's weights and values (include/de_hip.h de_eval_loss): real weights; Float32 sums of binary16 terms
loss_weight_type(::Type{T}) where {T<:Real} = T
loss_weight_type(::Type{Complex{T}}) where {T} = T
loss_value_type(::Type{T}) where {T<:Real} = T
loss_value_type(::Type{Float16}) = Float32
loss_value_type(::Type{Complex{T}}) where {T} = T

"""
    eval_population_loss(pop, X, y; weights=nothing, loss=:L2, loss_param=0.0) -> (loss::Vector{T}, ok)

`sum(abs2, trees[t](X) .- y)` (test/test_optim.jl:95,99) for every tree, reduced on the device:
the `N × n_trees` output matrix is never written.  `loss[t]` is NaN where `ok[t]` is false.
`loss` is `:L2`, `:L1` or a parameterised kind — `:huber` (δ), `:logcosh`, `:l1_eps` (ε), `:l2_eps` (ε), `:quantile` (τ), `:lp` (p),
`:logit_dist`, `:logit_margin`, `:l1_hinge` — with its parameter in `loss_param`.

A `Float16` or `Complex{T}` population made with `typed_loss=true` is served for `:L2` and `:L1` (DESIGN.md §4.4.17): the weights are
real (`Vector{Float16}` / `Vector{T}`), and the losses come back as `Vector{Float32}` (binary16 terms, summed in Float32) /
`Vector{T}` (`abs2` / `abs` of the complex residual).  Without `typed_loss` the library answers `DE_ERR_UNSUPPORTED` for them.
"""
function eval_population_loss(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{<:Real}}=nothing,
    loss::Symbol=:L2, loss_param::Real=0.0,
) where {T}
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    @assert weights === nothing || (eltype(weights) === loss_weight_type(T) && length(weights) == N)
    spec = loss_spec(loss, loss_param; with_gradient=false)
    out = Vector{loss_value_type(T)}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X y weights out ok ccall(
            (:de_eval_loss_ex, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec},
             Ptr{Cvoid}, Ptr{UInt8}),
            hc, hp, X, N, F, C_NULL, y, weights === nothing ? C_NULL : pointer(weights), spec, out, ok))
    end
    return out, ok .!= 0x00
end

# ---- minibatches (DESIGN.md §4.4.18; include/de_hip.h has the sampler's definition) -------------------------------------------------
struct BatchSrc             # de_batch_src_t
    X::Ptr{Cvoid}
    N::Int64
    ldX::Int64
    n_features::Int32
    classes_is_i64::Int32
    y::Ptr{Cvoid}
    w::Ptr{Cvoid}
    classes::Ptr{Cvoid}
end
struct BatchDst             # de_batch_dst_t
    X::Ptr{Cvoid}
    ldX::Int64
    y::Ptr{Cvoid}
    w::Ptr{Cvoid}
    classes::Ptr{Cvoid}
end
const BATCH_MODES = Dict{Symbol,Cint}(:replace => 0, :permute => 1)   # de_batch_mode_t

"""
    sample_population_rows(pop, N, n_rows; seed, step=0, mode=:replace, offset=0) -> Vector{Int64}

Positions `offset+1 … offset+n_rows` of the batch `(mode, N, seed, step)` as 1-based row indices into a dataset of `N` rows
(`de_batch_sample_rows`): a pure function of its arguments, the same rows on every machine and on the device.  `:replace` samples
with replacement, as SymbolicRegression.jl's `batching` does; `:permute` takes a slice of a keyed permutation of `1:N`
(`offset + n_rows <= N`): batches without replacement, epochs, train / hold-out splits.
"""
function sample_population_rows(
    pop::HIPPopulation, N::Integer, n_rows::Integer; seed::Integer, step::Integer=0, mode::Symbol=:replace, offset::Integer=0,
)
    haskey(BATCH_MODES, mode) || throw(ArgumentError("unknown batch mode $mode"))
    rows = Vector{Int64}(undef, n_rows)
    with_ctx(pop.ctx) do hc
        check(pop.ctx, GC.@preserve rows ccall(
            (:de_batch_sample_rows, LIBDE), Cint,
            (Ptr{Cvoid}, Cint, Int64, UInt64, UInt64, Int64, Int64, Ptr{Int64}),
            hc, BATCH_MODES[mode], N, seed % UInt64, step % UInt64, offset, n_rows, rows))
    end
    return rows .+ 1
end

"""
    gather_population_batch(pop, X, rows; y=nothing, weights=nothing, classes=nothing) -> (X=…, y=…, weights=…, classes=…, rows=rows)

The columns `rows` (1-based) of `X` and the same entries of `y`, `weights` and `classes` as a dense batch (`de_batch_gather`): every
`eval_population*` / `fit_population*` call takes it like any other dataset.  A row outside `1:N` is refused before anything is written.
"""
function gather_population_batch(
    pop::HIPPopulation{T}, X::Matrix{T}, rows::Vector{Int64};
    y::Union{Nothing,Vector{T}}=nothing, weights::Union{Nothing,Vector{<:Real}}=nothing, classes::Union{Nothing,Vector{Int64}}=nothing,
) where {T}
    F, N = size(X)
    n = length(rows)
    @assert y === nothing || length(y) == N
    @assert weights === nothing || (eltype(weights) === loss_weight_type(T) && length(weights) == N)
    @assert classes === nothing || length(classes) == N
    rows0 = rows .- 1
    Xb = Matrix{T}(undef, F, n)
    yb = y === nothing ? nothing : Vector{T}(undef, n)
    wb = weights === nothing ? nothing : Vector{loss_weight_type(T)}(undef, n)
    cb = classes === nothing ? nothing : Vector{Int64}(undef, n)
    p(v) = v === nothing ? C_NULL : Ptr{Cvoid}(pointer(v))
    with_ctx(pop.ctx) do hc
        check(pop.ctx, GC.@preserve X y weights classes rows0 Xb yb wb cb begin
            src = Ref(BatchSrc(p(X), N, max(F, 1), F, 1, p(y), p(weights), p(classes)))
            dst = Ref(BatchDst(p(Xb), max(F, 1), p(yb), p(wb), p(cb)))
            ccall((:de_batch_gather, LIBDE), Cint,
                (Ptr{Cvoid}, Cint, Ref{BatchSrc}, Ptr{Int64}, Int64, Ref{BatchDst}, Ptr{Int32}),
                hc, dtype_code(T), src, rows0, n, dst, C_NULL)
        end)
    end
    return (X=Xb, y=yb, weights=wb, classes=cb, rows=rows)
end

"""
    eval_population_loss_minibatch(pop, X, y, n_rows; seed, step=0, weights=nothing, loss=:L2, loss_param=0.0, mode=:replace, offset=0)
        -> (loss, ok, batch)

`sample_population_rows`, `gather_population_batch` and `eval_population_loss` on the batch: the stochastic scoring step of a search
on a large dataset.  A fit keeps one batch for its whole run: pass `batch.X, batch.y; weights=batch.weights` to `fit_population_*`.
"""
function eval_population_loss_minibatch(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}, n_rows::Integer; seed::Integer, step::Integer=0,
    weights::Union{Nothing,Vector{<:Real}}=nothing, loss::Symbol=:L2, loss_param::Real=0.0, mode::Symbol=:replace, offset::Integer=0,
) where {T}
    rows = sample_population_rows(pop, size(X, 2), n_rows; seed=seed, step=step, mode=mode, offset=offset)
    batch = gather_population_batch(pop, X, rows; y=y, weights=weights)
    out, ok = eval_population_loss(pop, batch.X, batch.y; weights=batch.weights, loss=loss, loss_param=loss_param)
    return out, ok, batch
end

"""
    eval_population_fit_stats(pop, X, y; weights=nothing) -> (stats::NamedTuple, ok)

The weighted second-order statistics of every tree's values `ŷ` against `y`, reduced on the device (`de_eval_fit_stats`; the
`N × n_trees` output matrix is never written).  `stats` holds, per tree, `mean_p`, `m2_p = Σ w (ŷ - mean_p)²` and
`cov = Σ w (ŷ - mean_p)(y - mean_y)` as `Vector{Float64}` (NaN where `ok[t]` is false), and the scalars `W = Σ w`, `mean_y`, `m2_y`.
Pearson's `r = cov / sqrt(m2_p * m2_y)`, the linear scaling `y ≈ a + b ŷ` with `b = cov / m2_p`, `a = mean_y - b * mean_p` and its
residual `m2_y - cov² / m2_p`, and `sum(abs2, ŷ .- y) = m2_y - 2cov + m2_p + W * (mean_p - mean_y)²` are functions of these.
A weight of zero excludes its sample.
"""
function eval_population_fit_stats(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{T}}=nothing,
) where {T}
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    @assert weights === nothing || length(weights) == N
    stats = Matrix{Float64}(undef, 3, pop.n_trees)
    ystats = Vector{Float64}(undef, 3)
    ok = Vector{UInt8}(undef, pop.n_trees)
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X y weights stats ystats ok ccall(
            (:de_eval_fit_stats, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64},
             Ptr{UInt8}),
            hc, hp, X, N, F, C_NULL, y, weights === nothing ? C_NULL : pointer(weights), stats, ystats, ok))
    end
    return (mean_p=stats[1, :], m2_p=stats[2, :], cov=stats[3, :], W=ystats[1], mean_y=ystats[2], m2_y=ystats[3]), ok .!= 0x00
end

"""
    set_population_constants!(pop, constants::Vector{T})

New constants for the trees of `pop`, same shapes: `constants` = the trees' `get_scalar_constants` vectors
(src/NodeUtils.jl:99-143: depth-first leaf order; a GraphNode's shared constant ONCE) back to back.  Nothing is
re-flattened or re-lowered — the immediates are patched inside the device programs (`de_program_set_consts`), which is
what an optimiser loop (`ext/DynamicExpressionsOptimExt.jl:182-224`) calls between `eval_population_loss_grad`
evaluations.  For a GraphNode population the values are fanned out to the occurrence slots of the library.
"""
function set_population_constants!(pop::HIPPopulation{T}, constants::Vector{T}) where {T}
    length(constants) == sum(pop.n_consts) || throw(ArgumentError("wrong number of constants"))
    vals = constants
    if any(o -> o !== nothing, pop.occ)          # one value per unique constant -> one per occurrence slot
        vals = Vector{T}(undef, sum(pop.n_slots))
        at, to = 0, 0
        for t in 1:pop.n_trees
            o = pop.occ[t]
            for k in 1:pop.n_slots[t]
                vals[to + k] = constants[at + (o === nothing ? k : o[k])]
            end
            at += pop.n_consts[t]; to += pop.n_slots[t]
        end
    end
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve vals ccall((:de_program_set_consts, LIBDE), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), hp, vals))
    end
    return pop
end

"""
    set_population_constants_device!(pop, ptr::Ptr{Cvoid})

The same from DEVICE memory (`de_program_set_consts_device`): `ptr` names `sum(pop.n_slots)` values of type `T` on the population's
device — the LIBRARY's layout, one value per occurrence slot (a GraphNode caller gathers its shared constants on the device first).  The
buffer is read in stream order on the context's stream; it may be reused as soon as that stream has passed the call.  Nothing is copied
to the host where the library can patch its streams on the device (`population_constants_on_device_path(pop)` says so); any other
program is staged through the host by the library itself.
"""
function set_population_constants_device!(pop::HIPPopulation{T}, ptr::Ptr{Cvoid}) where {T}
    with_pop(pop) do hc, hp
        check(pop.ctx, ccall((:de_program_set_consts_device, LIBDE), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), hp, ptr))
    end
    return pop
end
population_constants_on_device_path(pop::HIPPopulation) =
    with_pop(pop) do hc, hp
        ccall((:de_program_consts_device_path, LIBDE), Cint, (Ptr{Cvoid},), hp) == 1
    end

"""
    get_population_constants!(out::Vector{T}, pop) -> out

The current constants of `pop` in `set_population_constants!`'s layout (a GraphNode's shared constant once: its first occurrence),
from whichever side holds them (`de_program_get_consts`).
"""
function get_population_constants!(out::Vector{T}, pop::HIPPopulation{T}) where {T}
    length(out) == sum(pop.n_consts) || throw(ArgumentError("wrong number of constants"))
    vals = any(o -> o !== nothing, pop.occ) ? Vector{T}(undef, sum(pop.n_slots)) : out
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve vals ccall((:de_program_get_consts, LIBDE), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), hp, vals))
    end
    if vals !== out                              # one value per occurrence slot -> one per unique constant
        at, to = 0, 0
        for t in 1:pop.n_trees
            o = pop.occ[t]
            for k in pop.n_slots[t]:-1:1             # (descending: the FIRST occurrence is written last)
                out[at + (o === nothing ? k : o[k])] = vals[to + k]
            end
            at += pop.n_consts[t]; to += pop.n_slots[t]
        end
    end
    return out
end

grad_mode(variable) = variable isa Val{true} || variable === true ? Cint(0) : variable isa Val{:both} ? Cint(2) : Cint(1)
"""Gradient widths of the trees in the LIBRARY's layout (one row per occurrence slot) and their packed offsets."""
function grad_widths(hp::Ptr{Cvoid}, n_trees::Int, mode::Cint)
    ng = [ccall((:de_program_n_grad, LIBDE), Int64, (Ptr{Cvoid}, Int64, Cint), hp, t - 1, mode) for t in 1:n_trees]
    return ng, Int64[0; cumsum(ng)]
end

"""
    eval_population_loss_grad(pop, X, y; weights=nothing, loss=:L2, loss_param=0.0, variable=Val(false))
        -> (loss::Vector{T}, dloss::Vector{Vector{T}}, ok)

The optimiser callback of test/test_optim.jl:42-51 for a whole population in one launch:
`dloss[t][i] = sum_j 2 (ŷ_j - y_j) * dŷ_dconstants[i, j]` without the `n_grad × N` Jacobian.
`loss=:pullback` treats `y` as the cotangent `dY` of the ChainRules pullback
(src/ChainRules.jl:56-77) and returns its `dtree` gradient; the parameterised kinds of
`eval_population_loss` take their parameter in `loss_param`.
"""
function eval_population_loss_grad(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{T}}=nothing,
    loss::Symbol=:L2, loss_param::Real=0.0, variable=Val(false),
) where {T}
    mode = grad_mode(variable)
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    lossv = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    spec = loss_spec(loss, loss_param)
    dl, offs = with_pop(pop) do hc, hp
        ng, offs = grad_widths(hp, pop.n_trees, mode)
        dl = Vector{T}(undef, max(offs[end], 1))
        check(pop.ctx, GC.@preserve X y weights lossv dl offs ok ccall(
            (:de_eval_loss_grad_ex, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec},
             Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}),
            hc, hp, X, N, F, C_NULL, mode, y, weights === nothing ? C_NULL : pointer(weights), spec, lossv, dl, offs, ok))
        (dl, offs)
    end
    return lossv, [combine_rows(pop, t, dl[(offs[t] + 1):offs[t + 1]], mode) for t in 1:pop.n_trees], ok .!= 0x00
end

"""
    eval_population_gauss_newton(pop, X, y; weights=nothing, variable=Val(false), loss=:L2, loss_param=0.0, e_floor=1e-4, wide=false)
        -> (loss::Vector{T}, dloss::Vector{Vector{T}}, jtj::Vector{Matrix{T}}, ok, has_jtj)

The normal equations of a Levenberg-Marquardt step for a whole population in one launch (`de_eval_loss_gn_ex`): the loss `loss` and its
gradient exactly as `eval_population_loss_grad` returns them for the same kind, and `jtj[t] = sum_j w_j c_j d(j) d(j)'` over the gradient
rows of `variable`, without the `n_grad × N` Jacobian.  `c_j` is the kind's curvature weight (1 for `:L2`, where the Gauss-Newton Hessian
of the loss is `2 jtj[t]`; DESIGN.md §4.4.5) and `e_floor` the residual floor of the kinds whose weight is unbounded at a zero residual
(`:L1`, `:l1_eps`, `:quantile`, `:lp` with p < 2).  `:l1_hinge` (`DE_ERR_UNSUPPORTED`) and `:pullback` have no such matrix.  A tree of more than
`de_gn_max_rows()` rows in the library's per-occurrence layout has `has_jtj[t] == false` and a NaN matrix; its loss and gradient
are filled as usual.  For a GraphNode the rows and columns of a shared constant are summed (`combine_rows` on both sides).
`wide=true` (`de_eval_loss_gn_wide`, DESIGN.md §4.4.7) also forms the matrix of a tree of up to `de_gn_wide_max_rows()` = 32 rows; every
other output keeps the bits of the default call.  The library refuses it for a population with shared GraphNode subtrees.
"""
function eval_population_gauss_newton(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{T}}=nothing, variable=Val(false),
    loss::Symbol=:L2, loss_param::Real=0.0, e_floor::Real=1e-4, wide::Bool=false,
) where {T}
    mode = grad_mode(variable)
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    spec = loss_spec(loss, loss_param)
    lossv = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    dl, jt, ng, offs, joffs = with_pop(pop) do hc, hp
        ng, offs = grad_widths(hp, pop.n_trees, mode)
        joffs = Int64[0; cumsum(ng .* ng)]
        dl = Vector{T}(undef, max(offs[end], 1))
        jt = Vector{T}(undef, max(joffs[end], 1))
        wp = weights === nothing ? C_NULL : pointer(weights)
        if wide
            check(pop.ctx, GC.@preserve X y weights lossv dl jt offs joffs ok ccall(
                (:de_eval_loss_gn_wide, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Cdouble,
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}),
                hc, hp, X, N, F, C_NULL, mode, y, wp, spec, Float64(e_floor), lossv, dl, offs, jt, joffs, ok))
        else
            check(pop.ctx, GC.@preserve X y weights lossv dl jt offs joffs ok ccall(
                (:de_eval_loss_gn_ex, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Cdouble,
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}),
                hc, hp, X, N, F, C_NULL, mode, y, wp, spec, Float64(e_floor), lossv, dl, offs, jt, joffs, ok))
        end
        (dl, jt, ng, offs, joffs)
    end
    max_rows = wide ? ccall((:de_gn_wide_max_rows, LIBDE), Cint, ()) : ccall((:de_gn_max_rows, LIBDE), Cint, ())
    okb = ok .!= 0x00
    jtj = map(1:pop.n_trees) do t
        H = reshape(jt[(joffs[t] + 1):joffs[t + 1]], ng[t], ng[t])
        half = combine_rows(pop, t, H, mode)                              # S H
        Matrix(transpose(combine_rows(pop, t, Matrix(transpose(half)), mode)))   # (S (S H)')' = S H S'
    end
    return lossv, [combine_rows(pop, t, dl[(offs[t] + 1):offs[t + 1]], mode) for t in 1:pop.n_trees], jtj, okb,
           okb .& (ng .<= max_rows)
end

"""
    eval_population_fit_stats_grad(pop, X, y; weights=nothing, variable=Val(false), want_jtj=true, wide=false)
        -> (stats::NamedTuple, d_sum, d_pred, d_targ, jtj::Vector{Matrix{T}}, ok, has_jtj)

The fit statistics of `eval_population_fit_stats` with their gradients over the rows of `variable`, in one forward-dual launch
(`de_eval_fit_stats_grad`, DESIGN.md §4.4.6): per tree `d_sum[t] = D = Σ w d`, `d_pred[t] = P = Σ w (ŷ - mean_p) d`,
`d_targ[t] = Q = Σ w (y - mean_y) d` (`Vector{Float64}`) and `jtj[t] = Σ w d d'` (NaN where `has_jtj[t]` is false).  With
`b = cov / m2_p` the gradient of the residual under linear scaling is `2b (b P - Q)` and `b² (jtj - D D' / W - P P' / m2_p)` its
Gauss-Newton matrix with the scale and offset projected out.  For a GraphNode the rows of a shared constant are summed.
`wide=true` (`de_eval_fit_stats_grad_wide`, DESIGN.md §4.4.9) also forms the matrix of a tree of 9 to `de_gn_wide_max_rows()` = 32 rows —
the block of `eval_population_gauss_newton(wide=true)` under L2 — and keeps every other bit of the default call.
"""
function eval_population_fit_stats_grad(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{T}}=nothing, variable=Val(false),
    want_jtj::Bool=true, wide::Bool=false,
) where {T}
    mode = grad_mode(variable)
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    @assert weights === nothing || length(weights) == N
    stats = Matrix{Float64}(undef, 3, pop.n_trees)
    ystats = Vector{Float64}(undef, 3)
    ok = Vector{UInt8}(undef, pop.n_trees)
    dm, jt, ng, moffs, joffs = with_pop(pop) do hc, hp
        ng, offs = grad_widths(hp, pop.n_trees, mode)
        moffs = 3 .* offs
        joffs = Int64[0; cumsum(ng .* ng)]
        dm = Vector{Float64}(undef, max(moffs[end], 1))
        jt = fill(T(NaN), max(joffs[end], 1))
        if wide
            check(pop.ctx, GC.@preserve X y weights stats ystats dm jt moffs joffs ok ccall(
                (:de_eval_fit_stats_grad_wide, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}),
                hc, hp, X, N, F, C_NULL, mode, y, weights === nothing ? C_NULL : pointer(weights), stats, ystats,
                dm, moffs, want_jtj ? pointer(jt) : C_NULL, joffs, ok))
        else
            check(pop.ctx, GC.@preserve X y weights stats ystats dm jt moffs joffs ok ccall(
                (:de_eval_fit_stats_grad, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}),
                hc, hp, X, N, F, C_NULL, mode, y, weights === nothing ? C_NULL : pointer(weights), stats, ystats,
                dm, moffs, want_jtj ? pointer(jt) : C_NULL, joffs, ok))
        end
        (dm, jt, ng, moffs, joffs)
    end
    max_rows = wide ? ccall((:de_gn_wide_max_rows, LIBDE), Cint, ()) : ccall((:de_gn_max_rows, LIBDE), Cint, ())
    okb = ok .!= 0x00
    rows(q) = [combine_rows(pop, t, dm[(moffs[t] + q * ng[t] + 1):(moffs[t] + (q + 1) * ng[t])], mode) for t in 1:pop.n_trees]
    jtj = map(1:pop.n_trees) do t
        H = reshape(jt[(joffs[t] + 1):joffs[t + 1]], ng[t], ng[t])
        half = combine_rows(pop, t, H, mode)
        Matrix(transpose(combine_rows(pop, t, Matrix(transpose(half)), mode)))
    end
    st = (mean_p=stats[1, :], m2_p=stats[2, :], cov=stats[3, :], W=ystats[1], mean_y=ystats[2], m2_y=ystats[3])
    return st, rows(0), rows(1), rows(2), jtj, okb, okb .& (ng .<= max_rows) .& want_jtj
end

struct LmOpts               # de_lm_opts_t
    iters::Int32
    reserved::Int32
    lam0::Float64
    up::Float64
    down::Float64
    lam_min::Float64
end

"""
    population_lm_step(ctx, dloss::Vector{Vector{T}}, jtj::Vector{Matrix{T}}, has_jtj, lam) -> Vector{Vector{Float64}}

The Levenberg-Marquardt step of every tree on the device (`de_gn_lm_step`): `solve(H + lam_t * Diagonal(diag(H)), -g / 2)` by a
Cholesky factorisation in Float64, from what `eval_population_gauss_newton` returned (`lam`: a number or one value per tree).  The
zero vector where `has_jtj[t]` is false, the tree has no or more than `de_gn_max_rows()` rows, an entry is not finite or a pivot is not
positive — a rank-deficient matrix with `lam == 0` gives the zero step.
"""
function population_lm_step(
    ctx::HIPContext, dloss::Vector{Vector{T}}, jtj::Vector{Matrix{T}}, has_jtj::AbstractVector{Bool}, lam,
) where {T<:Union{Float32,Float64}}
    n = length(dloss)
    @assert length(jtj) == n && length(has_jtj) == n
    ng = Int32[length(g) for g in dloss]
    @assert all(size(jtj[t]) == (ng[t], ng[t]) for t in 1:n)
    offs = Int64[0; cumsum(Int64.(ng))]
    dl = T[v for g in dloss for v in g]
    jt = T[v for H in jtj for v in H]
    isempty(dl) && push!(dl, zero(T))
    isempty(jt) && push!(jt, zero(T))
    has = UInt8[h ? 0x01 : 0x00 for h in has_jtj]
    lams = lam isa Number ? fill(Float64(lam), n) : Vector{Float64}(lam)
    @assert length(lams) == n
    step = zeros(Float64, max(offs[end], 1))
    with_ctx(ctx) do hc
        check(ctx, GC.@preserve ng dl jt has lams step ccall(
            (:de_gn_lm_step, LIBDE), Cint,
            (Ptr{Cvoid}, Cint, Int64, Ptr{Int32}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}),
            hc, T === Float32 ? Cint(0) : Cint(1), n, ng, dl, C_NULL, jt, C_NULL, has, lams, step))
    end
    return [step[(offs[t] + 1):offs[t + 1]] for t in 1:n]
end

"""
    population_fit_stats_lm_step(ctx, stats, d_sum, d_pred, d_targ, jtj::Vector{Matrix{T}}, has_jtj, lam; wide=false)
        -> (steps::Vector{Vector{Float64}}, scaled_sse::Vector{Float64})

The Levenberg-Marquardt step of every tree under linear scaling on the device (`de_fit_stats_lm_step`, DESIGN.md §4.4.8), from what
`eval_population_fit_stats_grad` returned: the system `b² (jtj - D D' / W - P P' / m2_p)`, `2b (b P - Q)` is projected and solved
(`population_lm_step`'s Cholesky) in one kernel, in Float64.  The zero vector where `has_jtj[t]` is false, the tree has no or more than
`de_gn_max_rows()` rows, it is constant over the samples (`m2_p == 0`), an entry is not finite or a pivot is not positive.
`wide=true` (`de_fit_stats_lm_step_wide`, DESIGN.md §4.4.9) also solves the trees of 9 to 32 rows that
`eval_population_fit_stats_grad(wide=true)` formed the matrix of; a narrower tree keeps the default call's bytes.
"""
function population_fit_stats_lm_step(
    ctx::HIPContext, stats::NamedTuple, d_sum::Vector{Vector{Float64}}, d_pred::Vector{Vector{Float64}}, d_targ::Vector{Vector{Float64}},
    jtj::Vector{Matrix{T}}, has_jtj::AbstractVector{Bool}, lam; wide::Bool=false,
) where {T<:Union{Float32,Float64}}
    n = length(d_sum)
    @assert length(d_pred) == n && length(d_targ) == n && length(jtj) == n && length(has_jtj) == n && length(stats.mean_p) == n
    ng = Int32[length(g) for g in d_sum]
    @assert all(length(d_pred[t]) == ng[t] && length(d_targ[t]) == ng[t] && size(jtj[t]) == (ng[t], ng[t]) for t in 1:n)
    offs = Int64[0; cumsum(Int64.(ng))]
    st = Float64[v for t in 1:n for v in (stats.mean_p[t], stats.m2_p[t], stats.cov[t])]
    ys = Float64[stats.W, stats.mean_y, stats.m2_y]
    dm = Float64[v for t in 1:n for rows in (d_sum[t], d_pred[t], d_targ[t]) for v in rows]
    jt = T[v for H in jtj for v in H]
    isempty(st) && push!(st, 0.0)
    isempty(dm) && push!(dm, 0.0)
    isempty(jt) && push!(jt, zero(T))
    has = UInt8[h ? 0x01 : 0x00 for h in has_jtj]
    lams = lam isa Number ? fill(Float64(lam), n) : Vector{Float64}(lam)
    @assert length(lams) == n
    step = zeros(Float64, max(offs[end], 1))
    sse = Vector{Float64}(undef, max(n, 1))
    with_ctx(ctx) do hc
        if wide
            check(ctx, GC.@preserve ng st ys dm jt has lams step sse ccall(
                (:de_fit_stats_lm_step_wide, LIBDE), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                hc, T === Float32 ? Cint(0) : Cint(1), n, ng, st, ys, dm, C_NULL, jt, C_NULL, has, lams, step, sse))
        else
            check(ctx, GC.@preserve ng st ys dm jt has lams step sse ccall(
                (:de_fit_stats_lm_step, LIBDE), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                hc, T === Float32 ? Cint(0) : Cint(1), n, ng, st, ys, dm, C_NULL, jt, C_NULL, has, lams, step, sse))
        end
    end
    return [step[(offs[t] + 1):offs[t + 1]] for t in 1:n], sse[1:n]
end

"""
The `tie` argument of the tied device fits (`de_fit_consts_*_tied`, DESIGN.md §4.4.16): one 0-based id per constant slot of `pop` — the
unique constant of the slot within its tree, in first-occurrence order (`occurrence_map`, 1-based there), the identity for a tree that
shares nothing.  `nothing` (the library's identity) when no constant of the population is shared.
"""
function tie_map(pop::HIPPopulation)
    any(o -> o !== nothing, pop.occ) || return nothing
    tie = Int32[]
    for t in 1:pop.n_trees
        o = pop.occ[t]
        append!(tie, o === nothing ? (Int32(0):Int32(pop.n_slots[t] - 1)) : Int32.(o .- 1))
    end
    return tie
end

"""
    fit_population_constants_lm!(pop, X, y; weights=nothing, iters=10, lam0=1e-3, up=10.0, down=0.1, loss=:L2, loss_param=0.0, e_floor=1e-4,
                                 wide=false, scaled=false, tied=false)
        -> (constants::Vector{T}, loss::Vector{T}, ok, history::Matrix{Float64}, n_accept::Vector{Int32})

Levenberg-Marquardt on the constants of every tree at once, the whole loop in one library call (`de_fit_consts_lm_ex`), minimising the loss
kind `loss` (the keywords of `eval_population_gauss_newton`; the damped generalised Gauss-Newton step of DESIGN.md §4.4.5): it starts from the
constants `pop` holds (`set_population_constants!`), and per iteration solves the damped normal equations on the device, sets the trial
constants there, evaluates, and accepts a tree's step when its loss decreased (`lam_t *= down`, floor 1e-12; else `lam_t *= up`).
Afterwards `pop` holds the accepted constants, which are returned with their losses and flags; `history[:, r]` are the accepted losses
after `r - 1` iterations.  Trees that are incomplete at the start or wider than `de_gn_max_rows()` keep their constants.  A population
with a shared GraphNode constant is refused (its occurrence rows need folding) unless `tied=true` (`de_fit_consts_lm_tied`, DESIGN.md
§4.4.16): a shared constant is then ONE unknown, the occurrence rows and the matrix (`S H Sᵀ`) are folded on the device, and a tree is
fitted where it has at most `de_gn_max_rows()` occurrence slots; not with `wide` or `scaled`.
`wide=true` (`de_fit_consts_lm_wide`, DESIGN.md §4.4.7) also fits the trees of 9 to `de_gn_wide_max_rows()` = 32 constants; a narrower tree
follows the default call's trajectory bit for bit.
`scaled=true` (`de_fit_consts_lm_scaled`, DESIGN.md §4.4.8; `loss=:L2` only; with `wide=true` `de_fit_consts_lm_scaled_wide`, §4.4.9: trees of up
to 32 constants, a narrower tree on the default call's trajectory bit for bit) fits under Keijzer's linear scaling `a + b ŷ`:
the objective is `scaled_sse = m2_y - cov² / m2_p`, every evaluation `de_eval_fit_stats_grad`'s.  It returns
`(constants, scaled_sse::Vector{Float64}, ok, history, n_accept, stats)` with `stats` the NamedTuple of `eval_population_fit_stats_grad` at the
accepted constants (slope `cov / m2_p`, intercept `mean_y - slope * mean_p`).
"""
function fit_population_constants_lm!(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{T}}=nothing,
    iters::Integer=10, lam0::Real=1e-3, up::Real=10.0, down::Real=0.1, loss::Symbol=:L2, loss_param::Real=0.0, e_floor::Real=1e-4,
    wide::Bool=false, scaled::Bool=false, tied::Bool=false,
) where {T}
    tied && (wide || scaled) && throw(ArgumentError("fit_population_constants_lm!(tied=true): the scaled and the wide fits are not served under ties"))
    scaled && loss !== :L2 && throw(ArgumentError("fit_population_constants_lm!(scaled=true) minimises the L2 residual under linear scaling: loss $loss is not supported"))
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    @assert weights === nothing || length(weights) == N
    !tied && any(o -> o !== nothing, pop.occ) && throw(ArgumentError("fit_population_constants_lm!: shared GraphNode constants need tied=true or the host loop"))
    opts = Ref(LmOpts(Int32(iters), Int32(0), Float64(lam0), Float64(up), Float64(down), 1e-12))
    if scaled
        sse = Vector{Float64}(undef, pop.n_trees)
        stats = Matrix{Float64}(undef, 3, pop.n_trees)
        ystats = fill(NaN, 3)
        oks = Vector{UInt8}(undef, pop.n_trees)
        hist = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
        acc = zeros(Int32, pop.n_trees)
        with_pop(pop) do hc, hp
            if wide
                check(pop.ctx, GC.@preserve X y weights sse stats ystats oks hist acc ccall(
                    (:de_fit_consts_lm_scaled_wide, LIBDE), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LmOpts},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                    hc, hp, X, N, F, C_NULL, y, weights === nothing ? C_NULL : pointer(weights), opts, sse, stats, ystats, oks, hist, acc))
            else
                check(pop.ctx, GC.@preserve X y weights sse stats ystats oks hist acc ccall(
                    (:de_fit_consts_lm_scaled, LIBDE), Cint,
                    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LmOpts},
                     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                    hc, hp, X, N, F, C_NULL, y, weights === nothing ? C_NULL : pointer(weights), opts, sse, stats, ystats, oks, hist, acc))
            end
        end
        consts = get_population_constants!(Vector{T}(undef, sum(pop.n_consts)), pop)
        st = (mean_p=stats[1, :], m2_p=stats[2, :], cov=stats[3, :], W=ystats[1], mean_y=ystats[2], m2_y=ystats[3])
        return consts, sse, oks .!= 0x00, hist, acc, st
    end
    spec = loss_spec(loss, loss_param)
    lossv = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    history = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
    n_accept = zeros(Int32, pop.n_trees)
    with_pop(pop) do hc, hp
        wp = weights === nothing ? C_NULL : pointer(weights)
        if tied
            tie = tie_map(pop)
            check(pop.ctx, GC.@preserve X y weights tie lossv ok history n_accept ccall(
                (:de_fit_consts_lm_tied, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Cdouble, Ref{LmOpts},
                 Ptr{Int32}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, Float64(e_floor), opts, tie === nothing ? C_NULL : pointer(tie), lossv, ok, history, n_accept))
        elseif wide
            check(pop.ctx, GC.@preserve X y weights lossv ok history n_accept ccall(
                (:de_fit_consts_lm_wide, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Cdouble, Ref{LmOpts},
                 Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, Float64(e_floor), opts, lossv, ok, history, n_accept))
        else
            check(pop.ctx, GC.@preserve X y weights lossv ok history n_accept ccall(
                (:de_fit_consts_lm_ex, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Cdouble, Ref{LmOpts},
                 Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, Float64(e_floor), opts, lossv, ok, history, n_accept))
        end
    end
    constants = get_population_constants!(Vector{T}(undef, sum(pop.n_consts)), pop)
    return constants, lossv, ok .!= 0x00, history, n_accept
end

struct BfgsOpts             # de_bfgs_opts_t
    iters::Int32
    reserved::Int32
    step0::Float64
    shrink::Float64
    c1::Float64
    curv::Float64
end

"""
    fit_population_constants_bfgs!(pop, X, y; weights=nothing, iters=20, step0=1.0, shrink=0.5, c1=1e-4, curv=1e-8, loss=:L2, loss_param=0.0,
                                   scaled=false, tied=false)
        -> (constants::Vector{T}, loss::Vector{T}, ok, history::Matrix{Float64}, n_accept::Vector{Int32})

BFGS on the constants of every tree at once, the whole loop in one library call (`de_fit_consts_bfgs`, DESIGN.md §4.4.10) — the reference's
`optimize(f, g!, tree, BFGS())` with a backtracking line search, from the loss and its gradient alone: every kind of
`eval_population_loss_grad` except `:pullback` is an objective (`:l1_hinge` included), and every tree of up to `de_bfgs_max_rows()` = 32
constants is fitted.  It starts from the constants `pop` holds; per iteration the direction `-B g`, the trial constants, the evaluation
there, the Armijo accept rule and the update of `B` run on the device.  Afterwards `pop` holds the accepted constants, which are returned
with their losses and flags; `history[:, r]` are the accepted losses after `r - 1` iterations.  Trees that are incomplete at the start,
have no constants or more than 32 keep their constants.  A population with a shared GraphNode constant is refused unless `tied=true`
(`de_fit_consts_bfgs_tied`, DESIGN.md §4.4.16): a shared constant is then ONE unknown, its occurrence rows summed on the device, and a tree
of up to 32 UNIQUE constants is fitted; not with `scaled`.
`scaled=true` (`de_fit_consts_bfgs_scaled`, DESIGN.md §4.4.14; `loss=:L2` only) fits under Keijzer's linear scaling `a + b ŷ`: the objective is
`scaled_sse = m2_y - cov² / m2_p` and its gradient from the moments of `de_eval_fit_stats_grad` without a matrix, both in Float64.  It returns
`(constants, scaled_sse::Vector{Float64}, ok, history, n_accept, stats)` with `stats` the NamedTuple of `fit_population_constants_lm!(scaled=true)`
at the accepted constants.  A tree with a constant that is redundant under scaling, which the scaled Levenberg-Marquardt fit leaves alone, is fitted.
"""
function fit_population_constants_bfgs!(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{T}}=nothing,
    iters::Integer=20, step0::Real=1.0, shrink::Real=0.5, c1::Real=1e-4, curv::Real=1e-8, loss::Symbol=:L2, loss_param::Real=0.0,
    scaled::Bool=false, tied::Bool=false,
) where {T}
    tied && scaled && throw(ArgumentError("fit_population_constants_bfgs!(tied=true): the scaled fit is not served under ties"))
    scaled && loss !== :L2 && throw(ArgumentError("fit_population_constants_bfgs!(scaled=true) minimises the L2 residual under linear scaling: loss $loss is not supported"))
    loss === :pullback && throw(ArgumentError("fit_population_constants_bfgs!: :pullback is the cotangent of a pullback, not an objective"))
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    @assert weights === nothing || length(weights) == N
    !tied && any(o -> o !== nothing, pop.occ) && throw(ArgumentError("fit_population_constants_bfgs!: shared GraphNode constants need tied=true or the host loop"))
    opts = Ref(BfgsOpts(Int32(iters), Int32(0), Float64(step0), Float64(shrink), Float64(c1), Float64(curv)))
    if scaled
        sse = Vector{Float64}(undef, pop.n_trees)
        stats = Matrix{Float64}(undef, 3, pop.n_trees)
        ystats = fill(NaN, 3)
        oks = Vector{UInt8}(undef, pop.n_trees)
        hist = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
        acc = zeros(Int32, pop.n_trees)
        with_pop(pop) do hc, hp
            check(pop.ctx, GC.@preserve X y weights sse stats ystats oks hist acc ccall(
                (:de_fit_consts_bfgs_scaled, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{BfgsOpts},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, weights === nothing ? C_NULL : pointer(weights), opts, sse, stats, ystats, oks, hist, acc))
        end
        consts = get_population_constants!(Vector{T}(undef, sum(pop.n_consts)), pop)
        st = (mean_p=stats[1, :], m2_p=stats[2, :], cov=stats[3, :], W=ystats[1], mean_y=ystats[2], m2_y=ystats[3])
        return consts, sse, oks .!= 0x00, hist, acc, st
    end
    spec = loss_spec(loss, loss_param)
    lossv = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    history = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
    n_accept = zeros(Int32, pop.n_trees)
    with_pop(pop) do hc, hp
        wp = weights === nothing ? C_NULL : pointer(weights)
        if tied
            tie = tie_map(pop)
            check(pop.ctx, GC.@preserve X y weights tie lossv ok history n_accept ccall(
                (:de_fit_consts_bfgs_tied, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ref{BfgsOpts},
                 Ptr{Int32}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, opts, tie === nothing ? C_NULL : pointer(tie), lossv, ok, history, n_accept))
        else
            check(pop.ctx, GC.@preserve X y weights lossv ok history n_accept ccall(
                (:de_fit_consts_bfgs, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ref{BfgsOpts},
                 Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, opts, lossv, ok, history, n_accept))
        end
    end
    constants = get_population_constants!(Vector{T}(undef, sum(pop.n_consts)), pop)
    return constants, lossv, ok .!= 0x00, history, n_accept
end

struct LbfgsOpts            # de_lbfgs_opts_t
    iters::Int32
    reserved::Int32
    memory::Int32
    reserved2::Int32
    step0::Float64
    shrink::Float64
    c1::Float64
    curv::Float64
end

"""
    fit_population_constants_lbfgs!(pop, X, y; weights=nothing, iters=20, memory=8, step0=1.0, shrink=0.5, c1=1e-4, curv=1e-8, loss=:L2, loss_param=0.0,
                                    tied=false)
        -> (constants::Vector{T}, loss::Vector{T}, ok, history::Matrix{Float64}, n_accept::Vector{Int32})

L-BFGS on the constants of every tree at once, the whole loop in one library call (`de_fit_consts_lbfgs`, DESIGN.md §4.4.15) — the
reference's `optimize(f, g!, tree, LBFGS())` with a backtracking line search — for the trees `fit_population_constants_bfgs!` leaves
alone: every tree of up to `de_lbfgs_max_rows()` = 4096 constants is fitted, its curvature a ring of `memory` (1 .. 16) pairs instead of
`B`.  Arguments, objectives and results as `fit_population_constants_bfgs!`; the returned losses and flags are those of one fused loss
evaluation at the accepted constants (`eval_population_loss` there reproduces them bit for bit), `history` keeps the accept rule's.
`tied=true` (`de_fit_consts_lbfgs_tied`, DESIGN.md §4.4.16) serves a population with a shared GraphNode constant: ONE unknown per constant.
"""
function fit_population_constants_lbfgs!(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{T}}=nothing,
    iters::Integer=20, memory::Integer=8, step0::Real=1.0, shrink::Real=0.5, c1::Real=1e-4, curv::Real=1e-8, loss::Symbol=:L2,
    loss_param::Real=0.0, tied::Bool=false,
) where {T}
    loss === :pullback && throw(ArgumentError("fit_population_constants_lbfgs!: :pullback is the cotangent of a pullback, not an objective"))
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    @assert weights === nothing || length(weights) == N
    !tied && any(o -> o !== nothing, pop.occ) && throw(ArgumentError("fit_population_constants_lbfgs!: shared GraphNode constants need tied=true or the host loop"))
    opts = Ref(LbfgsOpts(Int32(iters), Int32(0), Int32(memory), Int32(0), Float64(step0), Float64(shrink), Float64(c1), Float64(curv)))
    spec = loss_spec(loss, loss_param)
    lossv = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    history = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
    n_accept = zeros(Int32, pop.n_trees)
    with_pop(pop) do hc, hp
        wp = weights === nothing ? C_NULL : pointer(weights)
        if tied
            tie = tie_map(pop)
            check(pop.ctx, GC.@preserve X y weights tie lossv ok history n_accept ccall(
                (:de_fit_consts_lbfgs_tied, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ref{LbfgsOpts},
                 Ptr{Int32}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, opts, tie === nothing ? C_NULL : pointer(tie), lossv, ok, history, n_accept))
        else
            check(pop.ctx, GC.@preserve X y weights lossv ok history n_accept ccall(
                (:de_fit_consts_lbfgs, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ref{LbfgsOpts},
                 Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, opts, lossv, ok, history, n_accept))
        end
    end
    constants = get_population_constants!(Vector{T}(undef, sum(pop.n_consts)), pop)
    return constants, lossv, ok .!= 0x00, history, n_accept
end

struct NmOpts               # de_nm_opts_t
    iters::Int32
    reserved::Int32
    a::Float64
    b::Float64
    f_tol::Float64
end

"""
    fit_population_constants_nm!(pop, X, y; weights=nothing, iters=200, a=0.025, b=0.5, f_tol=0.0, loss=:L2, loss_param=0.0, scaled=false, tied=false)
        -> (constants::Vector{T}, loss::Vector{T}, ok, history::Matrix{Float64}, n_improve::Vector{Int32})

Nelder-Mead on the constants of every tree at once, the whole loop in one library call (`de_fit_consts_nm`, DESIGN.md §4.4.13) — the
reference's `optimize(f, tree)` (test/test_optim.jl:6), which passes no gradient and so runs Optim's default method.  It needs the fused
loss alone: every kind of `eval_population_loss` is an objective, and a constant under `round`, `floor`, `sign`, ... moves.  It starts
from the constants `pop` holds; `iters` counts rounds of one evaluation each, the `G` rounds that build a tree's start simplex (`a`, `b`)
included.  Afterwards `pop` holds the accepted constants, which are returned with their losses and flags; `history[:, r]` are the
accepted losses after `r - 1` rounds and never increase; `n_improve` counts the rounds that lowered them.  Trees that are incomplete at
the start, have no constants or more than `de_nm_max_rows()` = 32 keep their constants.  A population with a shared GraphNode constant is
refused (the library moves every occurrence on its own) unless `tied=true` (`de_fit_consts_nm_tied`, DESIGN.md §4.4.16): ask and tell then
work on the unique constants, which are fanned out to their slots before every install; not with `scaled`.
`scaled=true` (`de_fit_consts_nm_scaled`, DESIGN.md §4.4.14; `loss=:L2` only) fits under Keijzer's linear scaling `a + b ŷ`: every evaluation is
`de_eval_fit_stats`, the objective `scaled_sse = m2_y - cov² / m2_p` in Float64.  It returns
`(constants, scaled_sse::Vector{Float64}, ok, history, n_improve, stats)` with `stats` the NamedTuple of `fit_population_constants_lm!(scaled=true)`
at the accepted constants.
"""
function fit_population_constants_nm!(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}; weights::Union{Nothing,Vector{T}}=nothing,
    iters::Integer=200, a::Real=0.025, b::Real=0.5, f_tol::Real=0.0, loss::Symbol=:L2, loss_param::Real=0.0,
    scaled::Bool=false, tied::Bool=false,
) where {T}
    tied && scaled && throw(ArgumentError("fit_population_constants_nm!(tied=true): the scaled fit is not served under ties"))
    scaled && loss !== :L2 && throw(ArgumentError("fit_population_constants_nm!(scaled=true) minimises the L2 residual under linear scaling: loss $loss is not supported"))
    loss === :pullback && throw(ArgumentError("fit_population_constants_nm!: :pullback is the cotangent of a pullback, not an objective"))
    F, N = size(X)
    @assert F >= pop.n_features && length(y) == N
    @assert weights === nothing || length(weights) == N
    !tied && any(o -> o !== nothing, pop.occ) && throw(ArgumentError("fit_population_constants_nm!: shared GraphNode constants need tied=true or the host loop"))
    opts = Ref(NmOpts(Int32(iters), Int32(0), Float64(a), Float64(b), Float64(f_tol)))
    if scaled
        sse = Vector{Float64}(undef, pop.n_trees)
        stats = Matrix{Float64}(undef, 3, pop.n_trees)
        ystats = fill(NaN, 3)
        oks = Vector{UInt8}(undef, pop.n_trees)
        hist = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
        acc = zeros(Int32, pop.n_trees)
        with_pop(pop) do hc, hp
            check(pop.ctx, GC.@preserve X y weights sse stats ystats oks hist acc ccall(
                (:de_fit_consts_nm_scaled, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{NmOpts},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, weights === nothing ? C_NULL : pointer(weights), opts, sse, stats, ystats, oks, hist, acc))
        end
        consts = get_population_constants!(Vector{T}(undef, sum(pop.n_consts)), pop)
        st = (mean_p=stats[1, :], m2_p=stats[2, :], cov=stats[3, :], W=ystats[1], mean_y=ystats[2], m2_y=ystats[3])
        return consts, sse, oks .!= 0x00, hist, acc, st
    end
    spec = loss_spec(loss, loss_param; with_gradient=false)
    lossv = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    history = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
    n_improve = zeros(Int32, pop.n_trees)
    with_pop(pop) do hc, hp
        wp = weights === nothing ? C_NULL : pointer(weights)
        if tied
            tie = tie_map(pop)
            check(pop.ctx, GC.@preserve X y weights tie lossv ok history n_improve ccall(
                (:de_fit_consts_nm_tied, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ref{NmOpts},
                 Ptr{Int32}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, opts, tie === nothing ? C_NULL : pointer(tie), lossv, ok, history, n_improve))
        else
            check(pop.ctx, GC.@preserve X y weights lossv ok history n_improve ccall(
                (:de_fit_consts_nm, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ref{NmOpts},
                 Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, C_NULL, y, wp, spec, opts, lossv, ok, history, n_improve))
        end
    end
    constants = get_population_constants!(Vector{T}(undef, sum(pop.n_consts)), pop)
    return constants, lossv, ok .!= 0x00, history, n_improve
end

"""
    eval_population_loss_grad_by_class(pop, X, y, parameters, classes; weights=nothing, loss=:L2, loss_param=0.0, variable=Val(:both))
        -> (loss, dloss::Vector{Vector{T}}, dparameters::Vector{Matrix{T}}, ok)

Parametric population: the fused loss gradient with the parameter rows reduced BY CLASS —
`dparameters[t]` is the gradient w.r.t. the `n_params × n_classes` parameter matrix, i.e. Zygote's
`grad.metadata._data.parameters` (test/test_parametric_expression.jl:326-372; the optimiser vector is
`vcat(constants, parameters[:])`, src/ParametricExpression.jl:260-265).  The library reduces class by
class over sample ranges, so the samples are ordered by class here (`sortperm`, stable); a search loop
that keeps its dataset ordered passes `grouped=true`.
"""
function eval_population_loss_grad_by_class(
    pop::HIPPopulation{T}, X::Matrix{T}, y::Vector{T}, parameters::Matrix{T}, classes::Vector{Int64};
    weights::Union{Nothing,Vector{T}}=nothing, loss::Symbol=:L2, loss_param::Real=0.0, variable=Val(:both), grouped::Bool=false,
) where {T}
    mode = variable isa Val{true} || variable === true ? Cint(0) : Cint(2)
    F, N = size(X)
    P, C = size(parameters)
    @assert F >= pop.n_features && length(y) == N && length(classes) == N
    @assert isempty(classes) || (minimum(classes) >= 1 && maximum(classes) <= C)   # src/ParametricExpression.jl:378-379 (the library trusts the ids)
    if !grouped
        perm = sortperm(classes; alg=MergeSort)
        X, y, classes = X[:, perm], y[perm], classes[perm]
        weights = weights === nothing ? nothing : weights[perm]
    end
    starts = zeros(Int64, C + 1)
    for c in classes
        starts[c + 1] += 1
    end
    cumsum!(starts, starts)
    lossv = Vector{T}(undef, pop.n_trees)
    dp = Array{T,3}(undef, P, C, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    spec = loss_spec(loss, loss_param)
    dl, offs = with_pop(pop) do hc, hp
        ng, offs = grad_widths(hp, pop.n_trees, mode)
        dl = Vector{T}(undef, max(offs[end], 1))
        check(pop.ctx, GC.@preserve X y weights parameters classes starts lossv dl dp offs ok begin
            pa = Ref(ParamArgs(pointer(parameters), P, C, pointer(classes), 1, 1))
            ccall((:de_eval_loss_grad_by_class_ex, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{ParamArgs}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec},
                 Ptr{Int64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{UInt8}),
                hc, hp, X, N, F, pa, mode, y, weights === nothing ? C_NULL : pointer(weights), spec, starts, lossv, dl, offs,
                dp, ok)
        end)
        (dl, offs)
    end
    return lossv, [combine_rows(pop, t, dl[(offs[t] + 1):offs[t + 1]], mode) for t in 1:pop.n_trees],
           [dp[:, :, t] for t in 1:pop.n_trees], ok .!= 0x00
end

# ---- per-tree parameter matrices (include/de_hip.h de_eval*_tree_params, DESIGN.md §4.4.11) ------------------------------------------
# Every ParametricExpression owns its parameter matrix (`metadata.parameters`, n_params × n_classes); `eval_population(pop, X,
# parameters, classes)` above reads ONE matrix for all trees.  Inside one class segment a parameter is a constant of its tree: the trees
# are rewritten by `de_tape_params_to_consts` into ordinary trees in which some constant slots stand for parameters (`slot_param`), and
# a call serves the population one class at a time, the slots patched on the device — the mirror of api.py's `ParametricPopulation`.
struct TreeParams           # de_tree_params_t
    params::Ptr{Cvoid}
    ld_params::Int64
    n_classes::Int64
    n_params::Int32
    reserved::Int32
    class_starts::Ptr{Int64}
    slot_param::Ptr{Int32}
end

mutable struct HIPParametricPopulation{T}
    pop::HIPPopulation{T}                # the rewritten trees: an ordinary population, n_params = 0
    slot_param::Vector{Int32}            # per constant slot of `pop`: -1 a real constant, else the 0-based parameter row
    slot_off::Vector{Int64}              # n_trees + 1: first slot of every tree
    n_params::Int
    parameters::Array{T,3}               # n_params × n_classes × n_trees: the expressions' own matrices
end

"""
    HIPParametricPopulation(exprs::Vector{<:ParametricExpression}, n_features; eval_context=EvalContext())

A population of `ParametricExpression`s that each carry their own parameters.  Tapes are flattened as `HIPPopulation` does, rewritten by
`de_tape_params_to_consts` and handed to `de_program_create` with `n_params = 0`.
"""
function HIPParametricPopulation(
    exprs::AbstractVector{<:ParametricExpression{T}}, n_features::Integer; eval_context::EvalContext=EvalContext(),
) where {T<:Union{Float32,Float64}}
    isempty(exprs) && error("empty population")
    operators = get_metadata(first(exprs)).operators
    optable = opcode_table(operators)
    P, C = size(get_metadata(first(exprs)).parameters)
    nodes, consts, slot_param = TapeNode[], T[], Int32[]
    node_off, const_off = Int64[0], Int64[0]
    parameters = Array{T,3}(undef, P, C, length(exprs))
    ctx = task_context()
    for (t, ex) in enumerate(exprs)
        size(get_metadata(ex).parameters) == (P, C) || error("the expressions differ in the shape of their parameters")
        parameters[:, :, t] .= get_metadata(ex).parameters
        tape, tconsts = TapeNode[], T[]
        flatten!(tape, tconsts, get_contents(ex), optable, 0)
        sp = Vector{Int32}(undef, length(tape))
        n = with_ctx(ctx) do _   # (a host-only hook; every library call of the shim goes under the context's lock)
            GC.@preserve tape sp ccall((:de_tape_params_to_consts, LIBDE), Int64,
                (Ptr{TapeNode}, Int64, Int32, Ptr{TapeNode}, Ptr{Int32}, Int64), tape, length(tape), P, tape, sp, length(sp))
        end
        n < 0 && error("de_tape_params_to_consts: status $(-n) (6: a parameter row >= n_params, 7: a shared subtree)")
        resize!(sp, n)
        k = 0                                   # the constant pool in slot order: the tree's constants, 0 in parameter slots
        for r in sp
            push!(consts, r < 0 ? tconsts[k += 1] : zero(T))
        end
        append!(nodes, tape); append!(slot_param, sp)
        push!(node_off, length(nodes)); push!(const_off, length(consts))
    end
    h = Ref{Ptr{Cvoid}}(C_NULL)
    with_ctx(ctx) do hc
        check(ctx, GC.@preserve nodes consts node_off const_off ccall(
            (:de_program_create, LIBDE), Cint,
            (Ptr{Cvoid}, Cint, Ptr{TapeNode}, Ptr{Int64}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int32, Int32, UInt32, Ref{Ptr{Cvoid}}),
            hc, dtype_code(T), nodes, node_off, length(exprs), consts, const_off, n_features, 0,
            option_bits(operators, eval_context), h))
    end
    n_slots = Int.(diff(const_off))
    pop = HIPPopulation{T}(ctx, h[], length(exprs), n_features, fill(nothing, length(exprs)), n_slots, copy(n_slots), optable)
    finalizer(finalize_population, pop)
    return HIPParametricPopulation{T}(pop, slot_param, const_off, P, parameters)
end

# the data ordered by class (stable) and the class_starts of de_tree_params_t
function group_by_class(X::Matrix{T}, classes::Vector{Int64}, C::Int, grouped::Bool, vecs...) where {T}
    @assert isempty(classes) || (minimum(classes) >= 1 && maximum(classes) <= C)   # src/ParametricExpression.jl:378-379
    perm = grouped ? nothing : sortperm(classes; alg=MergeSort)
    if perm !== nothing
        X, classes = X[:, perm], classes[perm]
        vecs = map(v -> v === nothing ? nothing : v[perm], vecs)
    end
    starts = zeros(Int64, C + 1)
    for c in classes
        starts[c + 1] += 1
    end
    cumsum!(starts, starts)
    return X, starts, perm, vecs
end

"""
    eval_parametric_population(pp, X, classes; parameters=pp.parameters, grouped=false) -> (out::Matrix{T}(N × n_trees), ok)

Every expression on every sample with ITS OWN parameters (`de_eval_tree_params`); `parameters` is `n_params × n_classes × n_trees`.
Columns of `out` are the reference's `Vector{T}(N)` results in the order of `X`.
"""
function eval_parametric_population(
    pp::HIPParametricPopulation{T}, X::Matrix{T}, classes::Vector{Int64}; parameters::Array{T,3}=pp.parameters, grouped::Bool=false,
) where {T}
    pop = pp.pop
    F, N = size(X)
    P, C, nt = size(parameters)
    @assert F >= pop.n_features && length(classes) == N && P == pp.n_params && nt == pop.n_trees
    X, starts, perm, _ = group_by_class(X, classes, C, grouped)
    out = Matrix{T}(undef, N, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    sp = pp.slot_param
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X parameters starts sp out ok begin
            tp = Ref(TreeParams(pointer(parameters), max(P, 1), C, P, 0, pointer(starts), pointer(sp)))
            ccall((:de_eval_tree_params, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{TreeParams}, Ptr{Cvoid}, Int64, Ptr{UInt8}),
                hc, hp, X, N, F, tp, out, N, ok)
        end)
    end
    if perm !== nothing
        out[perm, :] = out
    end
    return out, ok .!= 0x00
end

"""
    eval_parametric_population_loss(pp, X, y, classes; parameters, weights=nothing, loss=:L2, loss_param=0.0, grouped=false) -> (loss, ok)

`eval_population_loss` for expressions that each carry their own parameters (`de_eval_loss_tree_params`).
"""
function eval_parametric_population_loss(
    pp::HIPParametricPopulation{T}, X::Matrix{T}, y::Vector{T}, classes::Vector{Int64}; parameters::Array{T,3}=pp.parameters,
    weights::Union{Nothing,Vector{T}}=nothing, loss::Symbol=:L2, loss_param::Real=0.0, grouped::Bool=false,
) where {T}
    pop = pp.pop
    F, N = size(X)
    P, C, nt = size(parameters)
    @assert F >= pop.n_features && length(y) == N && length(classes) == N && P == pp.n_params && nt == pop.n_trees
    X, starts, _, (y, weights) = group_by_class(X, classes, C, grouped, y, weights)
    spec = loss_spec(loss, loss_param; with_gradient=false)
    out = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    sp = pp.slot_param
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X y weights parameters starts sp out ok begin
            tp = Ref(TreeParams(pointer(parameters), max(P, 1), C, P, 0, pointer(starts), pointer(sp)))
            ccall((:de_eval_loss_tree_params, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{TreeParams}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ptr{Cvoid},
                 Ptr{UInt8}),
                hc, hp, X, N, F, tp, y, weights === nothing ? C_NULL : pointer(weights), spec, out, ok)
        end)
    end
    return out, ok .!= 0x00
end

"""
    eval_parametric_population_loss_grad(pp, X, y, classes; parameters, weights=nothing, loss=:L2, loss_param=0.0, grouped=false)
        -> (loss, dconstants::Vector{Vector{T}}, dparameters::Vector{Matrix{T}}, ok)

The fused loss, its gradient w.r.t. every expression's real constants (`get_scalar_constants` order without the parameters) and
w.r.t. its own `n_params × n_classes` parameter matrix (`de_eval_loss_grad_tree_params`): `vcat(dconstants[t], dparameters[t][:])` is the
gradient of the optimiser's combined vector (src/ParametricExpression.jl:258-278).
"""
function eval_parametric_population_loss_grad(
    pp::HIPParametricPopulation{T}, X::Matrix{T}, y::Vector{T}, classes::Vector{Int64}; parameters::Array{T,3}=pp.parameters,
    weights::Union{Nothing,Vector{T}}=nothing, loss::Symbol=:L2, loss_param::Real=0.0, grouped::Bool=false,
) where {T}
    pop = pp.pop
    F, N = size(X)
    P, C, nt = size(parameters)
    @assert F >= pop.n_features && length(y) == N && length(classes) == N && P == pp.n_params && nt == pop.n_trees
    X, starts, _, (y, weights) = group_by_class(X, classes, C, grouped, y, weights)
    spec = loss_spec(loss, loss_param)
    lossv = Vector{T}(undef, pop.n_trees)
    dl = Vector{T}(undef, max(length(pp.slot_param), 1))
    dp = Array{T,3}(undef, P, C, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    sp, offs = pp.slot_param, pp.slot_off
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X y weights parameters starts sp offs lossv dl dp ok begin
            tp = Ref(TreeParams(pointer(parameters), max(P, 1), C, P, 0, pointer(starts), pointer(sp)))
            ccall((:de_eval_loss_grad_tree_params, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{TreeParams}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ptr{Cvoid},
                 Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}, Ptr{UInt8}),
                hc, hp, X, N, F, tp, y, weights === nothing ? C_NULL : pointer(weights), spec, lossv, dl, offs, dp, ok)
        end)
    end
    dconsts = [T[dl[s] for s in (offs[t] + 1):offs[t + 1] if sp[s] < 0] for t in 1:pop.n_trees]
    return lossv, dconsts, [dp[:, :, t] for t in 1:pop.n_trees], ok .!= 0x00
end

"""
    fit_parametric_population_bfgs!(pp, X, y, classes; parameters=pp.parameters, weights=nothing, iters=20, step0=1.0, shrink=0.5,
                                    c1=1e-4, curv=1e-8, loss=:L2, loss_param=0.0, grouped=false)
        -> (constants::Vector{Vector{T}}, parameters::Array{T,3}, loss::Vector{T}, ok, history::Matrix{Float64}, n_accept::Vector{Int32})

BFGS over every expression's `vcat(constants, parameters[:])` — the vector the reference optimises
(test/test_parametric_expression.jl:140-199) — the whole loop in one library call (`de_fit_tree_params_bfgs`, DESIGN.md §4.4.12).  The
real constants start from what `pp` holds, the parameters from `parameters`; afterwards `pp` holds the accepted constants and
`pp.parameters` the accepted parameters, which are returned with their losses and flags; `history[:, r]` are the accepted losses after
`r - 1` iterations.  An expression with more than `de_bfgs_max_rows()` = 32 unknowns, without unknowns or incomplete at the start keeps
its values.
"""
function fit_parametric_population_bfgs!(
    pp::HIPParametricPopulation{T}, X::Matrix{T}, y::Vector{T}, classes::Vector{Int64}; parameters::Array{T,3}=pp.parameters,
    weights::Union{Nothing,Vector{T}}=nothing, iters::Integer=20, step0::Real=1.0, shrink::Real=0.5, c1::Real=1e-4, curv::Real=1e-8,
    loss::Symbol=:L2, loss_param::Real=0.0, grouped::Bool=false,
) where {T}
    loss === :pullback && throw(ArgumentError("fit_parametric_population_bfgs!: :pullback is the cotangent of a pullback, not an objective"))
    pop = pp.pop
    F, N = size(X)
    P, C, nt = size(parameters)
    @assert F >= pop.n_features && length(y) == N && length(classes) == N && P == pp.n_params && nt == pop.n_trees
    @assert weights === nothing || length(weights) == N
    X, starts, _, (y, weights) = group_by_class(X, classes, C, grouped, y, weights)
    opts = Ref(BfgsOpts(Int32(iters), Int32(0), Float64(step0), Float64(shrink), Float64(c1), Float64(curv)))
    spec = loss_spec(loss, loss_param)
    fitted = copy(parameters)               # params_out: the start is read before anything is written, so it may be the same block
    lossv = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    history = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
    n_accept = zeros(Int32, pop.n_trees)
    sp, offs = pp.slot_param, pp.slot_off
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X y weights fitted starts sp lossv ok history n_accept begin
            tp = Ref(TreeParams(pointer(fitted), max(P, 1), C, P, 0, pointer(starts), pointer(sp)))
            ccall((:de_fit_tree_params_bfgs, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{TreeParams}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ref{BfgsOpts},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, tp, y, weights === nothing ? C_NULL : pointer(weights), spec, opts, fitted, lossv, ok, history, n_accept)
        end)
    end
    slots = get_population_constants!(Vector{T}(undef, length(sp)), pop)
    constants = [T[slots[s] for s in (offs[t] + 1):offs[t + 1] if sp[s] < 0] for t in 1:pop.n_trees]
    pp.parameters = fitted
    return constants, fitted, lossv, ok .!= 0x00, history, n_accept
end

"""
    fit_parametric_population_lbfgs!(pp, X, y, classes; parameters=pp.parameters, weights=nothing, iters=20, memory=8, step0=1.0,
                                     shrink=0.5, c1=1e-4, curv=1e-8, loss=:L2, loss_param=0.0, grouped=false)
        -> (constants::Vector{Vector{T}}, parameters::Array{T,3}, loss::Vector{T}, ok, history::Matrix{Float64}, n_accept::Vector{Int32})

L-BFGS over every expression's `vcat(constants, parameters[:])`, the whole loop in one library call (`de_fit_tree_params_lbfgs`, DESIGN.md
§4.4.15): `fit_parametric_population_bfgs!` for expressions of up to `de_lbfgs_max_rows()` = 4096 unknowns — `n_real + n_params *
n_classes` passes 32 with a handful of classes — with a ring of `memory` (1 .. 16) pairs per expression.  Arguments and results as
`fit_parametric_population_bfgs!`.
"""
function fit_parametric_population_lbfgs!(
    pp::HIPParametricPopulation{T}, X::Matrix{T}, y::Vector{T}, classes::Vector{Int64}; parameters::Array{T,3}=pp.parameters,
    weights::Union{Nothing,Vector{T}}=nothing, iters::Integer=20, memory::Integer=8, step0::Real=1.0, shrink::Real=0.5, c1::Real=1e-4,
    curv::Real=1e-8, loss::Symbol=:L2, loss_param::Real=0.0, grouped::Bool=false,
) where {T}
    loss === :pullback && throw(ArgumentError("fit_parametric_population_lbfgs!: :pullback is the cotangent of a pullback, not an objective"))
    pop = pp.pop
    F, N = size(X)
    P, C, nt = size(parameters)
    @assert F >= pop.n_features && length(y) == N && length(classes) == N && P == pp.n_params && nt == pop.n_trees
    @assert weights === nothing || length(weights) == N
    X, starts, _, (y, weights) = group_by_class(X, classes, C, grouped, y, weights)
    opts = Ref(LbfgsOpts(Int32(iters), Int32(0), Int32(memory), Int32(0), Float64(step0), Float64(shrink), Float64(c1), Float64(curv)))
    spec = loss_spec(loss, loss_param)
    fitted = copy(parameters)               # params_out: the start is read before anything is written, so it may be the same block
    lossv = Vector{T}(undef, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    history = Matrix{Float64}(undef, pop.n_trees, Int(iters) + 1)
    n_accept = zeros(Int32, pop.n_trees)
    sp, offs = pp.slot_param, pp.slot_off
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X y weights fitted starts sp lossv ok history n_accept begin
            tp = Ref(TreeParams(pointer(fitted), max(P, 1), C, P, 0, pointer(starts), pointer(sp)))
            ccall((:de_fit_tree_params_lbfgs, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ref{TreeParams}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{LossSpec}, Ref{LbfgsOpts},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Float64}, Ptr{Int32}),
                hc, hp, X, N, F, tp, y, weights === nothing ? C_NULL : pointer(weights), spec, opts, fitted, lossv, ok, history, n_accept)
        end)
    end
    slots = get_population_constants!(Vector{T}(undef, length(sp)), pop)
    constants = [T[slots[s] for s in (offs[t] + 1):offs[t + 1] if sp[s] < 0] for t in 1:pop.n_trees]
    pp.parameters = fitted
    return constants, fitted, lossv, ok .!= 0x00, history, n_accept
end

"""Forward-mode gradient of one tree: `(evaluation, gradient(n_grad × N), complete)` like
`eval_grad_tree_array(tree, cX, operators; variable)` (src/EvaluateDerivative.jl:193-228); a GraphNode's shared constant has
ONE row (the sum over its occurrences)."""
function _hip_eval_grad_tree_array(
    tree::AbstractExpressionNode{T}, cX::Matrix{T}, operators::OperatorEnum; variable=Val(false)
) where {T<:Union{Float16,Float32,Float64}}
    mode = grad_mode(variable)
    F, N = size(cX)
    pop = HIPPopulation([tree], operators, F; half_grad=(T === Float16))
    out = Vector{T}(undef, N)
    ok = Ref{UInt8}(0)
    grad = with_pop(pop) do hc, hp
        ng = ccall((:de_program_n_grad, LIBDE), Int64, (Ptr{Cvoid}, Int64, Cint), hp, 0, mode)
        grad = Matrix{T}(undef, ng, N)
        check(pop.ctx, GC.@preserve cX out grad ccall(
            (:de_eval_grad, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid},
             Ptr{Int64}, Ref{UInt8}),
            hc, hp, cX, N, F, C_NULL, mode, out, N, grad, C_NULL, ok))
        grad
    end
    return (out, combine_rows(pop, 1, grad, mode), ok[] != 0x00)
end

"""Single-direction derivative of one tree: `(evaluation, derivative, complete)` like
`eval_diff_tree_array(tree, cX, operators, direction)` (src/EvaluateDerivative.jl:40-53; `direction` is the
1-based feature, `complete` is always true on this path as in the reference, :68-119)."""
function _hip_eval_diff_tree_array(
    tree::AbstractExpressionNode{T}, cX::Matrix{T}, operators::OperatorEnum, direction::Integer
) where {T<:Union{Float16,Float32,Float64}}
    F, N = size(cX)
    1 <= direction <= F || throw(ArgumentError("direction must be a feature of cX"))
    pop = HIPPopulation([tree], operators, F; half_grad=(T === Float16))
    out = Vector{T}(undef, N)
    dout = Vector{T}(undef, N)
    ok = Ref{UInt8}(0)
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve cX out dout ccall(
            (:de_eval_diff, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{UInt8}),
            hc, hp, cX, N, F, Int32(direction - 1), out, dout, N, ok))
    end
    return (out, dout, ok[] != 0x00)
end

"""
    eval_population_pullback_dX(pop, X, dY) -> (dX::Array{T,3}(n_features × N × n_trees), ok)

The `dX` of the ChainRules pullback of `eval_tree_array` (`EvalPullback`, src/ChainRules.jl:56-77): `dX[:, :, t] =
dX_dY .* reshape(dY, 1, :)`, all-NaN where `ok[t]` is false (:62-64).  The `dtree` half is
`eval_population_loss_grad(pop, X, dY; loss=:pullback, variable=Val(false))`.
"""
function eval_population_pullback_dX(pop::HIPPopulation{T}, X::Matrix{T}, dY::Vector{T}) where {T}
    F, N = size(X)
    @assert F >= pop.n_features && length(dY) == N
    dX = Array{T,3}(undef, pop.n_features, N, pop.n_trees)
    ok = Vector{UInt8}(undef, pop.n_trees)
    with_pop(pop) do hc, hp
        check(pop.ctx, GC.@preserve X dY dX ok ccall(
            (:de_eval_pullback_dX, LIBDE), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}),
            hc, hp, X, N, F, C_NULL, dY, dX, C_NULL, ok))
    end
    return dX, ok .!= 0x00
end

# ---- multi-GPU: one Julia process per GPU (Distributed / MPI), RCCL through the library ----------------------------
"""
    HIPComm(ctx, rank, world, id)  /  hip_unique_id()

`de_dist_*` (include/de_hip.h "multi-GPU"): rank 0 calls `hip_unique_id()` and ships the 128 bytes to the other ranks
(`Distributed.remotecall`, MPI.Bcast ...); every rank builds `HIPComm(task_context(), rank, world, id)`, evaluates its
round-robin shard `trees[rank+1:world:end]`, and `gather_flags(comm, ok_local, n_trees)` returns the completion flags of
ALL trees in global order (one ncclAllGather over xGMI).  Outputs stay sharded.
"""
mutable struct HIPComm
    ctx::HIPContext
    handle::Ptr{Cvoid}
    rank::Int
    world::Int
end
function hip_unique_id()
    id = Vector{UInt8}(undef, 128)
    rc = ccall((:de_dist_unique_id, LIBDE), Cint, (Ptr{UInt8},), id)
    rc == DE_OK || error(unsafe_string(ccall((:de_dist_last_error, LIBDE), Cstring, (Ptr{Cvoid},), C_NULL)))
    return id
end
function HIPComm(ctx::HIPContext, rank::Integer, world::Integer, id::Vector{UInt8}=UInt8[])
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = with_ctx(ctx) do hc
        GC.@preserve id ccall((:de_dist_init, LIBDE), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Ref{Ptr{Cvoid}}),
                              hc, rank, world, world > 1 ? pointer(id) : C_NULL, h)
    end
    rc == DE_OK || error(unsafe_string(ccall((:de_dist_last_error, LIBDE), Cstring, (Ptr{Cvoid},), C_NULL)))
    return HIPComm(ctx, h[], rank, world)
end
function gather_flags(comm::HIPComm, ok_local::Vector{Bool}, n_trees::Integer)
    loc = UInt8.(ok_local)
    out = Vector{UInt8}(undef, n_trees)
    with_ctx(comm.ctx) do hc
        # the call only QUEUES its copies (host `loc` -> staging, gathered flags -> host `out`): both arrays must stay alive until
        # the stream has drained, so the synchronisation sits inside the same GC.@preserve (ADVICE r5)
        GC.@preserve loc out begin
            rc = ccall((:de_dist_gather_flags, LIBDE), Cint,
                (Ptr{Cvoid}, Ptr{UInt8}, Int64, Ptr{UInt8}), comm.handle, loc, n_trees, out)
            rc == DE_OK || error(unsafe_string(ccall((:de_dist_last_error, LIBDE), Cstring, (Ptr{Cvoid},), comm.handle)))
            check(comm.ctx, ccall((:de_ctx_synchronize, LIBDE), Cint, (Ptr{Cvoid},), hc))
        end
    end
    return out .!= 0x00
end
"""Bound every collective of `comm` (`de_dist_set_timeout`): the calls then wait for what they queued and fail with a message naming
the rank and the collective after `timeout_ms` instead of hanging on a peer that is down; 0 = asynchronous calls (the default)."""
function set_comm_timeout!(comm::HIPComm, timeout_ms::Integer)
    with_ctx(comm.ctx) do _
        rc = ccall((:de_dist_set_timeout, LIBDE), Cint, (Ptr{Cvoid}, Int64), comm.handle, timeout_ms)
        rc == DE_OK || error(unsafe_string(ccall((:de_dist_last_error, LIBDE), Cstring, (Ptr{Cvoid},), comm.handle)))
    end
    return nothing
end
close_comm(comm::HIPComm) = with_ctx(comm.ctx) do _
    comm.handle != C_NULL && ccall((:de_dist_destroy, LIBDE), Cint, (Ptr{Cvoid},), comm.handle)
    comm.handle = C_NULL
    nothing
end

is_extension_loaded(::Val{:HIP}) = true

end # module
