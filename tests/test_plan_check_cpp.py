"""The one-plan convenience of the plan check (direct_amd/host/poly_utils.hpp, polyhedronGenerator::checkTrajectory) compiles with the
node's own matrix and vector types and with the header's stand-ins.  No GPU needed: the unit is compiled and linked against
libdirect_ddp.so, not run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "%(root)s/tests/cpp/fake_data_type.h"              // stands for global_planner/utils/data_type.h
#include "%(root)s/direct_amd/host/poly_utils.hpp"
// after a sensor update: is the plan being flown still clear, and if not, when must the replan start?
double replanTime(direct::polyhedronGenerator& gen, const Eigen::MatrixXd& polyCoeff, const Eigen::VectorXd& polyTime, double t_now) {
  const direct::polyhedronGenerator::PlanCheck c = gen.checkTrajectory(polyCoeff, polyTime, 8, 0.0, t_now);
  if (c.clear()) return -1.0;
  return c.t_free + 0.0 * (c.segment + c.leaf + c.box[0] + c.box[5] + c.verdict);
}
int main() {
  direct::polyhedronGenerator gen(0.15, {{-3.0, -2.7, 0.0}}, 40, 36, 12);
  Eigen::MatrixXd poly(1, 18);
  Eigen::VectorXd T(1);
  direct::DenseMatrix pm(1, 18);
  direct::DenseVector pt(1);
  return (int)replanTime(gen, poly, T, 0.5) + gen.checkTrajectory(pm, pt).verdict + gen.checkTrajectory(pm, pt, 6, 0.2, -1.0, true).leaf;
}
'''


def test_check_convenience_compiles_next_to_reference_shaped_types(built, tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text(TU % {"root": ROOT})
    lib = os.path.join(ROOT, "direct_amd", "lib")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", str(src), "-o", str(tmp_path / "tu"),
                        "-L" + lib, "-ldirect_ddp", "-Wl,-rpath," + lib + ":/opt/rocm/lib",
                        "-Wl,--unresolved-symbols=ignore-in-shared-libs"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
