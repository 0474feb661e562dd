# test/runtests_hip_lm.jl — Levenberg-Marquardt on the constants on the device through the shim (DESIGN.md §4.4.4), run like
# ../runtests_hip.jl (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_lm.jl
using Test
using LinearAlgebra
using DynamicExpressions
using DynamicExpressions: Node, OperatorEnum

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt
@testset "Levenberg-Marquardt on the device (de_gn_lm_step, de_fit_consts_lm)" begin
    ops = OperatorEnum(; binary_operators=[+, -, *], unary_operators=[cos])
    x1 = Node{Float64}(; feature=1)
    tree = 1.7 * cos(x1 * 1.4) + 0.1
    X = reshape(collect(range(-2.0, 2.0; length=1_000)), 1, :)
    y = 2.0 .* cos.(1.5 .* X[1, :]) .- 0.5
    pop = HIP.HIPPopulation([tree], ops, 1)
    loss, dloss, jtj, ok, has = HIP.eval_population_gauss_newton(pop, X, y)
    step = HIP.population_lm_step(pop.ctx, dloss, jtj, has, 1e-3)
    want = (jtj[1] + 1e-3 * Diagonal(diag(jtj[1]))) \ (-dloss[1] ./ 2)
    @test isapprox(step[1], want; rtol=1e-10)
    @test all(iszero, HIP.population_lm_step(pop.ctx, dloss, jtj, [false], 1e-3)[1])
    constants, lossv, okv, history, n_accept = HIP.fit_population_constants_lm!(pop, X, y; iters=10)
    @test okv[1] && size(history) == (1, 11) && issorted(history[1, :]; rev=true) && n_accept[1] >= 3
    @test isapprox(constants, [2.0, 1.5, -0.5]; atol=1e-6)
    @test lossv[1] <= 1e-9 * loss[1]
    # the population holds the accepted constants
    l2, _, _ = HIP.eval_population_loss_grad(pop, X, y)
    @test l2 == lossv
end
