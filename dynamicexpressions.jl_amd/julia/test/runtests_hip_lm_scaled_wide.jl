# test/runtests_hip_lm_scaled_wide.jl — the scaled Levenberg-Marquardt fit for trees of 9 to 32 constants through the shim
# (DESIGN.md §4.4.9), run like ../runtests_hip.jl (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_lm_scaled_wide.jl
using Test
using LinearAlgebra
using DynamicExpressions
using DynamicExpressions: Node, OperatorEnum

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt
@testset "The scaled fit for wide trees (de_eval_fit_stats_grad_wide, de_fit_stats_lm_step_wide, de_fit_consts_lm_scaled_wide)" begin
    ops = OperatorEnum(; binary_operators=[+, -, *], unary_operators=[cos])
    xs = [Node{Float64}(; feature=f) for f in 1:3]
    cstar = [0.6 + 0.17 * i for i in 0:11]
    ramp = [0.12 * (i - 5.5) / 5.5 for i in 0:11]
    build(c) = sum(cos(c[i] * xs[1 + (i - 1) % 3]) for i in 1:12)   # cos_sum(12): twelve independent non-linear constants
    X = vcat((reshape(2.0 .* sin.(k .* collect(1.0:513.0)), 1, :) for k in (1.0, 1.7, 2.3))...)
    y = 2.0 .- 3.0 .* vec(sum(cos.(cstar .* X[[1 + (i - 1) % 3 for i in 1:12], :]); dims=1))
    pop = HIP.HIPPopulation([build(cstar .+ ramp)], ops, 3)
    st, D, P, Q, jtj, ok, has = HIP.eval_population_fit_stats_grad(pop, X, y; wide=true)
    st8, _, _, _, jtj8, _, has8 = HIP.eval_population_fit_stats_grad(pop, X, y)
    @test has[1] && !has8[1] && all(isnan, jtj8[1]) && all(isfinite, jtj[1]) && size(jtj[1]) == (12, 12) && st.cov == st8.cov
    steps, sse = HIP.population_fit_stats_lm_step(pop.ctx, st, D, P, Q, jtj, has, 1e-3; wide=true)
    b = st.cov[1] / st.m2_p[1]
    Ht = b^2 .* (jtj[1] .- D[1] * D[1]' ./ st.W .- P[1] * P[1]' ./ st.m2_p[1])
    g = 2b .* (b .* P[1] .- Q[1])
    @test isapprox(steps[1], (Ht + 1e-3 * Diagonal(diag(Ht))) \ (-g ./ 2); rtol=1e-6)
    @test sse[1] == st.m2_y - st.cov[1]^2 / st.m2_p[1]
    @test all(iszero, HIP.population_fit_stats_lm_step(pop.ctx, st, D, P, Q, jtj, has, 1e-3)[1][1])   # the narrow call: the zero step
    constants, sse_fit, okv, history, n_accept, stats = HIP.fit_population_constants_lm!(pop, X, y; iters=20, scaled=true, wide=true)
    @test okv[1] && size(history) == (1, 21) && issorted(history[1, :]; rev=true) && n_accept[1] >= 3
    @test sse_fit[1] <= max(1e-9 * history[1, 1], 4 * 1024 * 2.0^-53 * stats.m2_y)
    @test_throws ArgumentError HIP.fit_population_constants_lm!(pop, X, y; scaled=true, wide=true, loss=:huber, loss_param=1.0)
end
