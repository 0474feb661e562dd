# test/runtests_hip_tree_params.jl — expressions that each carry their own parameter matrix, through the shim (DESIGN.md §4.4.11), run
# like ../runtests_hip.jl (never executed in the builder's image, which has no Julia):
#
#     DE_HIP_LIB=/path/to/libde_hip.so julia --project=<env with DynamicExpressions> test/runtests_hip_tree_params.jl
using Test
using DynamicExpressions
using DynamicExpressions: ParametricExpression, OperatorEnum, parse_expression

include(joinpath(@__DIR__, "..", "DynamicExpressionsHIPExt.jl"))
const HIP = DynamicExpressionsHIPExt
@testset "per-tree parameter matrices (de_eval*_tree_params)" begin
    # the case of the reference's test/test_parametric_expression.jl:140-199
    true_parameters = [
        -0.2 +0.2 +0.3
        +1.4 +0.5 -0.9
    ]
    init_parameters = zero(true_parameters)
    X = [
        11 12 13 14 15 16 17 18 19.0
        21 22 23 24 25 26 27 28 29
    ]
    classes = [1, 2, 3, 3, 2, 1, 1, 2, 3]
    (init_ex, true_ex) = map(
        p -> parse_expression(
            :((x * p2) + y + p1);
            variable_names=["x", "y"],
            binary_operators=[+, -, *, /],
            unary_operators=[sin],
            expression_type=ParametricExpression,
            parameters=p,
            parameter_names=["p1", "p2"],
        ),
        (copy(init_parameters), copy(true_parameters)),
    )
    true_out = [X[1, i] * true_parameters[2, classes[i]] + X[2, i] + true_parameters[1, classes[i]] for i in 1:size(X, 2)]
    pp = HIP.HIPParametricPopulation([init_ex, true_ex], 2)
    @test pp.slot_param == Int32[1, 0, 1, 0] && pp.n_params == 2 && size(pp.parameters) == (2, 3, 2)

    # values: each expression with its own parameters, columns in the order of X
    out, ok = HIP.eval_parametric_population(pp, X, classes)
    @test all(ok) && out[:, 1] == init_ex(X, classes) && out[:, 2] == true_ex(X, classes) && out[:, 2] == true_out

    # loss and gradients: known answer at the zero parameters — e = yhat - y = -(x p2[c] + p1[c]) with the TRUE p
    lossv, okl = HIP.eval_parametric_population_loss(pp, X, true_out, classes)
    l2, dconsts, dparams, okg = HIP.eval_parametric_population_loss_grad(pp, X, true_out, classes)
    e = X[2, :] .- true_out
    @test all(okl) && all(okg) && lossv == l2 && lossv[2] == 0 && isapprox(lossv[1], sum(abs2, e))
    @test lossv[1] > 0.1                                  # the reference's init_loss (:198)
    @test all(isempty, dconsts) && all(iszero, dparams[2])
    want = zeros(2, 3)
    for i in 1:size(X, 2)
        want[1, classes[i]] += 2 * e[i]
        want[2, classes[i]] += 2 * e[i] * X[1, i]
    end
    @test isapprox(dparams[1], want)

    # other parameters for the same programs; an Inf in one expression's used column clears its flag alone
    swapped = cat(true_parameters, init_parameters; dims=3)
    out2, ok2 = HIP.eval_parametric_population(pp, X, classes; parameters=swapped)
    @test all(ok2) && out2[:, 1] == out[:, 2] && out2[:, 2] == out[:, 1]
    bad = copy(pp.parameters)
    bad[1, 2, 1] = Inf
    l3, ok3 = HIP.eval_parametric_population_loss(pp, X, true_out, classes; parameters=bad)
    @test !ok3[1] && isnan(l3[1]) && ok3[2] && l3[2] == 0
    # grouped data gives the same bits
    perm = sortperm(classes; alg=MergeSort)
    l4, _, dp4, _ = HIP.eval_parametric_population_loss_grad(pp, X[:, perm], true_out[perm], classes[perm]; grouped=true)
    @test l4 == l2 && dp4 == dparams

    # the reference's fit (:180-199) in one library call (de_fit_tree_params_bfgs, DESIGN.md §4.4.12): from zeros, 60 iterations
    consts, fitted, lf, okf, history, n_accept = HIP.fit_parametric_population_bfgs!(pp, X, true_out, classes; iters=60)
    @test all(okf) && all(isempty, consts) && size(history) == (2, 61) && pp.parameters === fitted
    @test history[1, 1] > 0.1 && lf[1] < 1e-5             # init_loss, result.minimum
    @test isapprox(fitted[:, :, 1], true_parameters; rtol=sqrt(eps(Float64)))
    @test lf[2] == 0 && fitted[:, :, 2] == true_parameters && n_accept[2] == 0 && n_accept[1] >= 3
    @test all(diff(history[1, :]) .<= 0)                  # only steps that lower the loss are taken
    l5, _, _, _ = HIP.eval_parametric_population_loss_grad(pp, X, true_out, classes)
    @test l5 == lf                                        # the evaluation at the result reproduces the loss
end
