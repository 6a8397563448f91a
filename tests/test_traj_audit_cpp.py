"""The one-plan convenience of the continuous-time audit (direct_amd/host/ddp_optimizer.hpp, auditTrajectory) compiles next to
a header shaped like the reference's data_type.h, with the node's own corridor, matrix and vector types.  No GPU needed: the
unit is compiled and linked against libdirect_ddp.so, not run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r'''
#include "%(root)s/tests/cpp/fake_data_type.h"              // stands for global_planner/utils/data_type.h
#include "%(root)s/direct_amd/host/ddp_optimizer.hpp"
static double _MAX_Vel = 2, _MAX_Acc = 2, _MAX_Jer = 10;
int acceptPlan(direct::DdpDevice& dev, const decomp_cvx_space::FlightCorridor& corridor, const Eigen::MatrixXd& polyCoeff,
               const Eigen::VectorXd& polyTime) {
  const direct::PlanAudit a = direct::auditTrajectory(dev, polyCoeff, polyTime, corridor, _MAX_Vel, _MAX_Acc, _MAX_Jer, 0.05);
  if (a.ok()) return 0;
  if (a.verdict & DIRECT_AUDIT_CORRIDOR) return 100 + a.c_segment + a.c_plane + (a.cpeak > 0) + (a.at[3] > 0);
  if (a.verdict & DIRECT_AUDIT_INVALID) return -1;
  return a.slowdown > 1.0 && a.vpeak + a.apeak + a.jpeak + a.vnorm + a.anorm + a.jnorm + a.gap[0] + a.t_total > 0 ? 1 : 2;
}
int main() {
  decomp_cvx_space::FlightCorridor c;
  decomp_cvx_space::Polytope p;
  Eigen::Vector4d h;
  h(3) = -1.0;
  p.appendPlane(h);
  c.appendPolytope(p);
  c.appendTime(1.0);
  Eigen::MatrixXd poly(1, 18);
  Eigen::VectorXd T(1);
  direct::PlainCorridor plain;                                   // and with the header's own stand-ins
  direct::DenseMatrix pm(1, 18);
  direct::DenseVector pt(1);
  direct::DdpDevice dev(1, 1, 6, DIRECT_F32);
  return acceptPlan(dev, c, poly, T) + direct::auditTrajectory(dev, pm, pt, plain, 2.0, 2.0, 0.0, 0.0, true).verdict;
}
'''


def test_audit_convenience_compiles_next_to_reference_shaped_types(built, tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text(TU % {"root": ROOT})
    lib = os.path.join(ROOT, "direct_amd", "lib")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", str(src), "-o", str(tmp_path / "tu"),
                        "-L" + lib, "-ldirect_ddp", "-Wl,-rpath," + lib + ":/opt/rocm/lib",
                        "-Wl,--unresolved-symbols=ignore-in-shared-libs"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
