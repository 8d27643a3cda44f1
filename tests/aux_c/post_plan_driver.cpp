// Host driver of the stages behind k_reconcile (isaac_ros_apriltag_amd/csrc/post_plan.h) for tests/test_post_plan_cpu.py.  One case
// per line on stdin, one result line per case on stdout; a mode is "NBUNDLES NRIGID ITERATIONS SIGMA NUNDIST":
//   plan  MODE N OSTRIDE      plan_post: the steps in order, "<kernel>:<gx>x<gy>><writes>" each
//   apply MODE WHAT VALUE     post_apply (WHAT: planar, rigid, refine, cov, undistort): "<new mode> | <key before> <key after> <retired>"
// A kernel is U (k_undistort_records), P (k_bundle_pose), R<cov> (k_bundle_rigid<cov>) or F<cov> (k_pose_refine<cov>); the pose
// launches carry "t" where they read the undistorted twins and "r" where they read the raw records.  A write is
// "<block>/<b|r><per_frame>": indexed frames x bundles (b) or frames x min(nout, ostride) records (r); several are joined by ",".
#include <iostream>
#include <sstream>
#include <string>

#include "../../isaac_ros_apriltag_amd/csrc/post_plan.h"

int main() {
  static const char* const kBlocks[] = {"udets", "bposes", "xposes", "xcovs", "rposes", "rcovs"};
  static const char* const kSettings[] = {"planar", "rigid", "refine", "cov", "undistort"};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    PostMode m;
    in >> cmd >> m.nbundles >> m.nrigid >> m.pose_iterations >> m.cov_sigma >> m.nundist;
    if (!in) { std::cout << "bad input\n"; return 1; }
    if (cmd == "plan") {
      uint32_t n = 0, ostride = 0;
      in >> n >> ostride;
      if (!in) { std::cout << "bad input\n"; return 1; }
      const PostPlan p = plan_post(m, n, ostride);
      for (int i = 0; i < p.nsteps; i++) {
        const PostStep& s = p.steps[i];
        std::cout << (i ? " " : "") << "UPRF"[s.kernel];
        if (s.kernel == POST_K_RIGID || s.kernel == POST_K_REFINE) std::cout << (s.cov ? 1 : 0);
        if (s.kernel != POST_K_UNDISTORT) std::cout << (s.twins ? 't' : 'r');
        std::cout << ':' << s.gx << 'x' << s.gy << '>';
        for (int j = 0; j < s.nwrites; j++)
          std::cout << (j ? "," : "") << kBlocks[s.writes[j].block] << '/' << (s.writes[j].index == POST_BY_BUNDLE ? 'b' : 'r') << s.writes[j].per_frame;
      }
      std::cout << '\n';
    } else {
      std::string what;
      double value = 0;
      in >> what >> value;
      int k = 0;
      while (k < 5 && what != kSettings[k]) k++;
      if (!in || k == 5) { std::cout << "bad input\n"; return 1; }
      const PostMode r = post_apply(m, (PostSetting)k, value);
      std::cout << r.nbundles << ' ' << r.nrigid << ' ' << r.pose_iterations << ' ' << r.cov_sigma << ' ' << r.nundist << " | "
                << post_graph_key(m) << ' ' << post_graph_key(r) << ' ' << (post_graph_key(m) != post_graph_key(r)) << '\n';
    }
  }
  return 0;
}
