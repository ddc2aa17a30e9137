// The same toy window as estimator_shim.cpp, written against include/tcv_ceres_shim.hpp: the statements have the shape of
// Estimator::OptimizationWithLine() (reference vins_estimator/src/estimator.cpp:1679-2046) with `ceres::` / the factor classes
// replaced by `tcvshim::`.
//
//   g++ -std=c++14 -Iinclude examples/estimator_shim_classes.cpp -Ltc-viml_amd -ltcv_hip -Wl,-rpath,$PWD/tc-viml_amd -o shim2
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>

#include "tcv_ceres_shim.hpp"

using namespace tcvshim;

int main() {
    if (tcv_device_count() < 1) { std::printf("no HIP device: nothing to run (the library has no CPU path)\n"); return 0; }
    double para_Pose[2][7] = {{0, 0, 0, 0, 0, 0, 1}, {0.1, 0, 0, 0, 0, 0, 1}};
    double para_SpeedBias[2][9] = {{1, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0, 0, 0, 0}};
    double para_Ex_Pose[1][7] = {{0, 0, 0, 0, 0, 0, 1}};
    double para_Feature[1][1] = {{0.2}};
    const double G[3] = {0, 0, 9.81007};
    tcv_imu_preintegration pre;
    std::memset(&pre, 0, sizeof pre);
    pre.delta_q[3] = 1.0; pre.sum_dt = 0.1;
    pre.delta_p[0] = 0.1; pre.delta_p[2] = 0.5 * 9.81007 * 0.01; pre.delta_v[2] = 9.81007 * 0.1;
    for (int i = 0; i < 15; i++) { pre.jacobian[16 * i] = 1.0; pre.covariance[16 * i] = 1e-4; }
    const double pts_i[3] = {0.0, 0.0, 1.0}, pts_j[3] = {-0.02, 0.0, 1.0};
    try {
        Solver::Summary summary;
        {
            Problem problem;                                                       // estimator.cpp:1679
            problem.SetGravity(G);
            LossFunction *loss_function = new CauchyLoss(1.0);                     // :1682
            for (int i = 0; i < 2; i++) {                                          // :1683-1688
                problem.AddParameterBlock(para_Pose[i], 7, new PoseLocalParameterization());
                problem.AddParameterBlock(para_SpeedBias[i], 9);
            }
            problem.AddParameterBlock(para_Ex_Pose[0], 7, new PoseLocalParameterization());      // :1689-1701
            problem.SetParameterBlockConstant(para_Ex_Pose[0]);
            problem.AddResidualBlock(new IMUFactor(pre), nullptr, para_Pose[0], para_SpeedBias[0], para_Pose[1], para_SpeedBias[1]);      // :1728-1731
            problem.AddResidualBlock(new ProjectionFactor(pts_i, pts_j), loss_function, para_Pose[0], para_Pose[1], para_Ex_Pose[0], para_Feature[0]);      // :1766
            Solver::Options options;                                               // :1888-1897
            options.linear_solver_type = SPARSE_SCHUR;
            options.trust_region_strategy_type = DOGLEG;
            options.max_num_iterations = 8;
            // Problem::Evaluate around the solve: the cost by factor family at the states before and after
            auto evaluate = [&](const char *when) {
                double cost = 0, fam[4];
                std::vector<double> residuals, gradient;
                if (!problem.Evaluate(Problem::EvaluateOptions(), &cost, &residuals, &gradient, fam)) throw std::runtime_error("Problem::Evaluate failed");
                std::printf("evaluate (%s): cost %.17g = prior %.17g + imu %.17g + points %.17g + lines %.17g; %d residuals, %d gradient entries\n", when, cost, fam[0],
                            fam[1], fam[2], fam[3], (int)residuals.size(), (int)gradient.size());
            };
            evaluate("before");
            Solve(options, &problem, &summary);                                    // :1900
            evaluate("after");
        }                                                                          // problem (and its factors) destroyed here, like :2119
        std::printf("solve: %d iterations, cost %.6g -> %.6g, inverse depth %.6f\n", (int)summary.iterations.size(), summary.initial_cost, summary.final_cost,
                    para_Feature[0][0]);

        // MARGIN_OLD, estimator.cpp:1911-2046
        CauchyLoss loss(1.0);
        MarginalizationInfo *marginalization_info = new MarginalizationInfo();
        marginalization_info->SetGravity(G);
        marginalization_info->addResidualBlockInfo(new ResidualBlockInfo(new IMUFactor(pre), nullptr,
            std::vector<double *>{para_Pose[0], para_SpeedBias[0], para_Pose[1], para_SpeedBias[1]}, std::vector<int>{0, 1}));                 // :1936-1942
        marginalization_info->addResidualBlockInfo(new ResidualBlockInfo(new ProjectionFactor(pts_i, pts_j), &loss,
            std::vector<double *>{para_Pose[0], para_Pose[1], para_Ex_Pose[0], para_Feature[0]}, std::vector<int>{0, 3}));                     // :1980-1986
        marginalization_info->preMarginalize();
        marginalization_info->marginalize();
        std::unordered_map<long, double *> addr_shift;                             // :2027-2039
        addr_shift[reinterpret_cast<long>(para_Pose[1])] = para_Pose[0];
        addr_shift[reinterpret_cast<long>(para_SpeedBias[1])] = para_SpeedBias[0];
        addr_shift[reinterpret_cast<long>(para_Ex_Pose[0])] = para_Ex_Pose[0];
        std::vector<double *> parameter_blocks = marginalization_info->getParameterBlocks(addr_shift);
        std::printf("prior: m = %d, n = %d, %d kept blocks, first -> para_Pose[0]: %s\n", marginalization_info->m, marginalization_info->n,
                    (int)parameter_blocks.size(), parameter_blocks[0] == para_Pose[0] ? "yes" : "no");

        // next window: the prior enters as a MarginalizationFactor (:1714-1720)
        {
            Problem problem;
            problem.SetGravity(G);
            problem.AddParameterBlock(para_Pose[0], 7, new PoseLocalParameterization());
            problem.AddParameterBlock(para_SpeedBias[0], 9);
            problem.AddResidualBlock(new MarginalizationFactor(marginalization_info), nullptr, parameter_blocks);
            Solver::Options options;
            options.max_num_iterations = 4;
            Solve(options, &problem, &summary);
            std::printf("prior-only window: cost %.6g -> %.6g\n", summary.initial_cost, summary.final_cost);
        }
        // ceres::Covariance (include/tcv_covariance.h): how well the IMU factor alone ties the newest pose to a fixed older frame.  (The
        // window above has no prior and no lines: nothing fixes its gauge, and Compute would report it rank deficient.)
        {
            Problem problem;
            problem.SetGravity(G);
            for (int i = 0; i < 2; i++) {
                problem.AddParameterBlock(para_Pose[i], 7, new PoseLocalParameterization());
                problem.AddParameterBlock(para_SpeedBias[i], 9);
            }
            problem.SetParameterBlockConstant(para_Pose[0]);
            problem.SetParameterBlockConstant(para_SpeedBias[0]);
            problem.AddResidualBlock(new IMUFactor(pre), nullptr, para_Pose[0], para_SpeedBias[0], para_Pose[1], para_SpeedBias[1]);
            problem.SetFrames({para_Pose[0], para_Pose[1]}, {para_SpeedBias[0], para_SpeedBias[1]});
            Covariance covariance;
            if (!covariance.Compute({{para_Pose[1], para_Pose[1]}, {para_Pose[1], para_SpeedBias[1]}}, &problem)) throw std::runtime_error("Covariance::Compute: rank deficient");
            double c6[36], c7[49], cross[6 * 9], cross_t[9 * 6];
            covariance.GetCovarianceBlockInTangentSpace(para_Pose[1], para_Pose[1], c6);
            covariance.GetCovarianceBlock(para_Pose[1], para_Pose[1], c7);
            covariance.GetCovarianceBlockInTangentSpace(para_Pose[1], para_SpeedBias[1], cross);
            covariance.GetCovarianceBlockInTangentSpace(para_SpeedBias[1], para_Pose[1], cross_t);
            bool zero_last = true, symmetric = true;
            for (int i = 0; i < 7; i++) zero_last = zero_last && c7[6 * 7 + i] == 0.0 && c7[i * 7 + 6] == 0.0;
            for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) symmetric = symmetric && c6[6 * i + j] == c6[6 * j + i] && c7[7 * i + j] == c6[6 * i + j];
            for (int i = 0; i < 6; i++) for (int j = 0; j < 9; j++) symmetric = symmetric && cross[9 * i + j] == cross_t[6 * j + i];
            std::printf("covariance of the newest pose: sigma_p %.6g %.6g %.6g sigma_theta %.6g %.6g %.6g; ambient 7 x 7 last row and column zero: %d; symmetric: %d\n",
                        std::sqrt(c6[0]), std::sqrt(c6[7]), std::sqrt(c6[14]), std::sqrt(c6[21]), std::sqrt(c6[28]), std::sqrt(c6[35]), (int)zero_last, (int)symmetric);
        }
        // ... and of a feature (include/tcv_landmark_covariance.h): the same window with the point factor, the extrinsic held constant
        {
            Problem problem;
            problem.SetGravity(G);
            for (int i = 0; i < 2; i++) {
                problem.AddParameterBlock(para_Pose[i], 7, new PoseLocalParameterization());
                problem.AddParameterBlock(para_SpeedBias[i], 9);
            }
            problem.AddParameterBlock(para_Ex_Pose[0], 7, new PoseLocalParameterization());
            problem.SetParameterBlockConstant(para_Pose[0]);
            problem.SetParameterBlockConstant(para_SpeedBias[0]);
            problem.SetParameterBlockConstant(para_Ex_Pose[0]);
            problem.AddResidualBlock(new IMUFactor(pre), nullptr, para_Pose[0], para_SpeedBias[0], para_Pose[1], para_SpeedBias[1]);
            problem.AddResidualBlock(new ProjectionFactor(pts_i, pts_j), new CauchyLoss(1.0), para_Pose[0], para_Pose[1], para_Ex_Pose[0], para_Feature[0]);
            problem.SetFrames({para_Pose[0], para_Pose[1]}, {para_SpeedBias[0], para_SpeedBias[1]});
            Covariance covariance;
            if (!covariance.Compute({{para_Feature[0], para_Feature[0]}, {para_Feature[0], para_Pose[1]}}, &problem)) throw std::runtime_error("Covariance::Compute: rank deficient");
            double var = 0.0, row[6], col7[7];
            covariance.GetCovarianceBlock(para_Feature[0], para_Feature[0], &var);
            covariance.GetCovarianceBlockInTangentSpace(para_Feature[0], para_Pose[1], row);
            covariance.GetCovarianceBlock(para_Pose[1], para_Feature[0], col7);
            std::printf("variance of the feature's inverse depth: %.6g (sigma %.6g at %.3g); with the newest pose's x: %.6g; ambient 7 x 1 last entry zero: %d\n", var, std::sqrt(var),
                        para_Feature[0][0], row[0], (int)(col7[6] == 0.0 && col7[0] == row[0]));
        }
        delete marginalization_info;
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
