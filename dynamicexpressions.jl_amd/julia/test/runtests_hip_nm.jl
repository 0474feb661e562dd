# test/runtests_hip_nm.jl — Nelder-Mead on the constants on the device through the shim (DESIGN.md §4.4.13), run like ../runtests_hip.jl
# (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_nm.jl
using Test
using Random: MersenneTwister
using DynamicExpressions
using DynamicExpressions: Node, OperatorEnum

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt
@testset "Nelder-Mead on the device (de_fit_consts_nm)" begin
    # the scenario of the reference's test/test_optim.jl, whose first fit, optimize(f, tree), passes no gradient
    ops = OperatorEnum(; binary_operators=[+, -, *, /], unary_operators=[exp])
    x1, x2 = Node{Float64}(; feature=1), Node{Float64}(; feature=2)
    X = rand(MersenneTwister(0), Float64, 2, 100)
    y = @. exp(X[1, :] * 2.1 - 0.9) + X[2, :] * -0.9
    tree = exp(x1 * 0.8 - 0.0) + 5.2 * x2
    pop = HIP.HIPPopulation([tree], ops, 2)
    loss0, _ = HIP.eval_population_loss(pop, X, y)
    constants, lossv, okv, history, n_improve = HIP.fit_population_constants_nm!(pop, X, y; iters=300)
    @test okv[1] && size(history) == (1, 301) && issorted(history[1, :]; rev=true) && n_improve[1] >= 3
    @test history[1, 1] == loss0[1] && lossv[1] < loss0[1]
    # the population holds the accepted constants
    l2, _ = HIP.eval_population_loss(pop, X, y)
    @test l2 == lossv
    @test_throws ArgumentError HIP.fit_population_constants_nm!(pop, X, y; loss=:pullback)
end
