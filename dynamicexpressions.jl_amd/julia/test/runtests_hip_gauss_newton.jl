# test/runtests_hip_gauss_newton.jl — the Gauss-Newton normal equations of the shim (DESIGN.md §4.4.3) against the reference's own CPU
# Jacobian, run like ../runtests_hip.jl (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_gauss_newton.jl
using Test
using LinearAlgebra
using DynamicExpressions
using DynamicExpressions: Node, OperatorEnum, eval_tree_array, eval_grad_tree_array

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt

@testset "Gauss-Newton normal equations (de_eval_loss_gn)" begin
    ops = OperatorEnum(; binary_operators=[+, -, *], unary_operators=[cos])
    x1, x2 = Node{Float64}(; feature=1), Node{Float64}(; feature=2)
    tree = 1.7 * cos(x1 * 1.4) - x2 * 0.5 + 0.25
    X = randn(Float64, 2, 1_000)
    y = 2.0 .* cos.(1.5 .* X[1, :]) .- 0.4 .* X[2, :]
    w = rand(Float64, 1_000) .+ 0.5
    w[1:7:end] .= 0.0
    pop = HIP.HIPPopulation([tree], ops, 2)
    p, J, _ = eval_grad_tree_array(tree, X, ops; variable=false)
    for weights in (nothing, w)
        ww = weights === nothing ? ones(1_000) : weights
        loss, dloss, jtj, ok, has = HIP.eval_population_gauss_newton(pop, X, y; weights=weights)
        @test ok[1] && has[1] && size(jtj[1]) == (4, 4)
        @test jtj[1] == transpose(jtj[1])
        @test isapprox(jtj[1], (J .* ww') * J'; rtol=1e-11)
        @test isapprox(dloss[1], J * (2 .* ww .* (p .- y)); rtol=1e-10, atol=1e-10)
        @test isapprox(loss[1], sum(ww .* (p .- y) .^ 2); rtol=1e-12)
        # the same loss and gradient as the gradient call, bit for bit
        l2, d2, _ = HIP.eval_population_loss_grad(pop, X, y; weights=weights)
        @test l2 == loss && d2 == dloss
        # one Gauss-Newton step lowers the loss
        step = (jtj[1] + 1e-3 * Diagonal(diag(jtj[1]))) \ (-dloss[1] ./ 2)
        @test norm(step) > 0
    end
end
