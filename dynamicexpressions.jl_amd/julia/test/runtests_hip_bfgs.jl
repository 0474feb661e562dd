# test/runtests_hip_bfgs.jl — BFGS on the constants on the device through the shim (DESIGN.md §4.4.10), run like ../runtests_hip.jl
# (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_bfgs.jl
using Test
using Random: MersenneTwister
using DynamicExpressions
using DynamicExpressions: Node, OperatorEnum

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt
@testset "BFGS on the device (de_fit_consts_bfgs)" begin
    # the scenario of the reference's test/test_optim.jl
    ops = OperatorEnum(; binary_operators=[+, -, *, /], unary_operators=[exp])
    x1, x2 = Node{Float64}(; feature=1), Node{Float64}(; feature=2)
    X = rand(MersenneTwister(0), Float64, 2, 100)
    y = @. exp(X[1, :] * 2.1 - 0.9) + X[2, :] * -0.9
    tree = exp(x1 * 0.8 - 0.0) + 5.2 * x2
    pop = HIP.HIPPopulation([tree], ops, 2)
    loss0, _, _ = HIP.eval_population_loss_grad(pop, X, y)
    constants, lossv, okv, history, n_accept = HIP.fit_population_constants_bfgs!(pop, X, y; iters=60)
    @test okv[1] && size(history) == (1, 61) && issorted(history[1, :]; rev=true) && n_accept[1] >= 3
    @test history[1, 1] == loss0[1]
    @test isapprox(constants[1], 2.1; atol=0.01)
    # the population holds the accepted constants
    l2, _, _ = HIP.eval_population_loss_grad(pop, X, y)
    @test l2 == lossv
    @test_throws ArgumentError HIP.fit_population_constants_bfgs!(pop, X, y; loss=:pullback)
end
