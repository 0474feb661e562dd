# test/runtests_hip_lm_scaled.jl — Levenberg-Marquardt on the constants under linear scaling on the device through the shim
# (DESIGN.md §4.4.8), run like ../runtests_hip.jl (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_lm_scaled.jl
using Test
using LinearAlgebra
using DynamicExpressions
using DynamicExpressions: Node, OperatorEnum

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt
@testset "Levenberg-Marquardt under linear scaling on the device (de_fit_stats_lm_step, de_fit_consts_lm_scaled)" begin
    ops = OperatorEnum(; binary_operators=[+, -, *], unary_operators=[cos])
    x1, x2 = Node{Float64}(; feature=1), Node{Float64}(; feature=2)
    tree = cos(1.69 * x1) + 0.49 * x2   # no constant absorbs scale or offset; started at theta* (1 + 0.3)
    X = vcat(reshape(collect(range(-2.0, 2.0; length=513)), 1, :), reshape(sin.(collect(1.0:513.0)), 1, :))
    y = 2.0 .- 3.0 .* (cos.(1.3 .* X[1, :]) .+ 0.7 .* X[2, :])
    pop = HIP.HIPPopulation([tree], ops, 2)
    st, D, P, Q, jtj, ok, has = HIP.eval_population_fit_stats_grad(pop, X, y)
    steps, sse = HIP.population_fit_stats_lm_step(pop.ctx, st, D, P, Q, jtj, has, 1e-3)
    b = st.cov[1] / st.m2_p[1]
    Ht = b^2 .* (jtj[1] .- D[1] * D[1]' ./ st.W .- P[1] * P[1]' ./ st.m2_p[1])
    g = 2b .* (b .* P[1] .- Q[1])
    @test isapprox(steps[1], (Ht + 1e-3 * Diagonal(diag(Ht))) \ (-g ./ 2); rtol=1e-9)
    @test sse[1] == st.m2_y - st.cov[1]^2 / st.m2_p[1]
    @test all(iszero, HIP.population_fit_stats_lm_step(pop.ctx, st, D, P, Q, jtj, [false], 1e-3)[1][1])
    constants, sse_fit, okv, history, n_accept, stats = HIP.fit_population_constants_lm!(pop, X, y; iters=10, scaled=true)
    @test okv[1] && size(history) == (1, 11) && issorted(history[1, :]; rev=true) && n_accept[1] >= 3
    @test sse_fit[1] <= max(1e-9 * history[1, 1], 4 * 1024 * 2.0^-53 * stats.m2_y)
    slope = stats.cov[1] / stats.m2_p[1]
    @test isapprox(slope, -3.0; atol=1e-4) && isapprox(stats.mean_y - slope * stats.mean_p[1], 2.0; atol=1e-4)
    # (scaled=true with wide=true is served since DESIGN.md §4.4.9: test/runtests_hip_lm_scaled_wide.jl)
    @test_throws ArgumentError HIP.fit_population_constants_lm!(pop, X, y; scaled=true, loss=:huber, loss_param=1.0)
end
