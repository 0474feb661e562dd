# test/runtests_hip_fit_stats.jl — the fit statistics of the shim (DESIGN.md §4.4.2) against the reference's own CPU path, run like
# ../runtests_hip.jl (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_fit_stats.jl
using Test
using DynamicExpressions
using DynamicExpressions: Node, OperatorEnum, eval_tree_array

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt

@testset "fit statistics (de_eval_fit_stats)" begin
    ops = OperatorEnum(; binary_operators=[+, -, *], unary_operators=[cos])
    x1, x2 = Node{Float64}(; feature=1), Node{Float64}(; feature=2)
    tree = x1 * 1.5 - cos(x2 * 0.5)
    X = randn(Float64, 2, 1_000)
    y = 2.0 .+ randn(Float64, 1_000)
    w = rand(Float64, 1_000) .+ 0.5
    w[1:7:end] .= 0.0
    pop = HIP.HIPPopulation([tree], ops, 2)
    p, _ = eval_tree_array(tree, X, ops)
    for weights in (nothing, w)
        ww = weights === nothing ? ones(1_000) : weights
        st, ok = HIP.eval_population_fit_stats(pop, X, y; weights=weights)
        W = sum(ww)
        mp, my = sum(ww .* p) / W, sum(ww .* y) / W
        @test ok[1] && isapprox(st.W, W; rtol=1e-14) && isapprox(st.mean_y, my; rtol=1e-13)
        @test isapprox(st.mean_p[1], mp; rtol=1e-12)
        @test isapprox(st.m2_p[1], sum(ww .* (p .- mp) .^ 2); rtol=1e-12)
        @test isapprox(st.m2_y, sum(ww .* (y .- my) .^ 2); rtol=1e-13)
        @test isapprox(st.cov[1], sum(ww .* (p .- mp) .* (y .- my)); rtol=1e-10, atol=1e-10)
        # the L2 loss from the moments
        @test isapprox(st.m2_y - 2st.cov[1] + st.m2_p[1] + W * (mp - my)^2, sum(ww .* (p .- y) .^ 2); rtol=1e-11)
    end
    # a target that is a linear function of the tree: slope, intercept, r = -1
    yl = 2.0 .- 3.0 .* p
    st, _ = HIP.eval_population_fit_stats(pop, X, yl)
    b = st.cov[1] / st.m2_p[1]
    @test isapprox(b, -3.0; rtol=1e-10) && isapprox(st.mean_y - b * st.mean_p[1], 2.0; rtol=1e-10)
    @test isapprox(st.cov[1] / sqrt(st.m2_p[1] * st.m2_y), -1.0; rtol=1e-12)
end
