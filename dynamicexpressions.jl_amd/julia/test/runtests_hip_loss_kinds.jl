# test/runtests_hip_loss_kinds.jl — the parameterised loss kinds of the shim (DESIGN.md §4.4.1) against the reference's own CPU path,
# run like ../runtests_hip.jl (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_loss_kinds.jl
using Test
using DynamicExpressions
using DynamicExpressions: Node, OperatorEnum, eval_tree_array, eval_grad_tree_array

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt

@testset "parameterised loss kinds (de_eval_loss_ex / de_eval_loss_grad_ex)" begin
    ops = OperatorEnum(; binary_operators=[+, -, *], unary_operators=[cos])
    x1, x2 = Node{Float64}(; feature=1), Node{Float64}(; feature=2)
    tree = x1 * 1.5 - cos(x2 * 0.5)
    X = randn(Float64, 2, 1_000)
    y = randn(Float64, 1_000)
    pop = HIP.HIPPopulation([tree], ops, 2)
    yh, _ = eval_tree_array(tree, X, ops)
    e = yh .- y
    _, gr, _ = eval_grad_tree_array(tree, X, ops; variable=Val(false))
    lh, okh = HIP.eval_population_loss(pop, X, y; loss=:huber, loss_param=1.3)
    @test okh[1] && isapprox(lh[1], sum(ifelse.(abs.(e) .<= 1.3, e .^ 2 ./ 2, 1.3 .* (abs.(e) .- 0.65))); rtol=1e-12)
    lq, dq, _ = HIP.eval_population_loss_grad(pop, X, y; loss=:quantile, loss_param=0.3)
    @test isapprox(lq[1], sum(e .* ((e .> 0) .- 0.3)); rtol=1e-12)
    @test isapprox(dq[1], vec(sum(((e .> 0) .- 0.3)' .* gr; dims=2)); rtol=1e-9)
    lc, _ = HIP.eval_population_loss(pop, X, y; loss=:logcosh)
    @test isapprox(lc[1], sum(log.(cosh.(e))); rtol=1e-12)
    @test_throws ArgumentError HIP.eval_population_loss(pop, X, y; loss=:pullback)
    @test_throws Exception HIP.eval_population_loss(pop, X, y; loss=:huber, loss_param=0.0)
end
