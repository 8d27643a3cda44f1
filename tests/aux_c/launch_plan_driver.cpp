// Host driver of the launch schedule (isaac_ros_apriltag_amd/csrc/launch_plan.h) for tests/test_launch_plan_cpu.py.  One case per
// line on stdin, one result line per case on stdout:
//   classes MCP SPLIT CUS B                                     plan_classes: per class "nt sort_cap lo hi grid slot_cap pop kernel",
//                                                               then "| prefilter_class"
//   layouts MCP SPLIT CUS B PCAP CCAP                           plan_work_layouts: its status, then per layout (all, latency) and
//                                                               class "lo hi off cap", then "| words"
//   plan    MCP SPLIT CUS B N W H HCAP PATH PREFILTER           plan_launch: "latency cc_waves border_per_wave cc_root_grid
//                                                               select_chunks select_grid decode_grid |" and the fit steps
// A fit step is "F" (fork), "P<nt>:grid:stream" (prefilter) or "C<class>:grid:pop:stream", with a "*" behind the class where it
// pops from the prefilter's compact list; stream "s" is the submission stream, 0 .. 2 the side streams.
#include <iostream>
#include <sstream>
#include <string>

#include "../../isaac_ros_apriltag_amd/csrc/launch_plan.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    int mcp = 0, split = 0;
    unsigned cus = 0;
    uint32_t B = 0;
    in >> cmd >> mcp >> split >> cus >> B;
    if (!in) { std::cout << "bad input\n"; return 1; }
    const FqClassTable t = plan_classes(mcp, split != 0, cus, B);
    if (cmd == "classes") {
      for (const FqClassSpec& c : t.cls)
        std::cout << c.nt << ' ' << c.sort_cap << ' ' << c.lo << ' ' << c.hi << ' ' << c.grid << ' ' << c.slot_cap << ' ' << c.pop << ' '
                  << c.kernel << " ; ";
      std::cout << "| " << t.prefilter_class << '\n';
    } else if (cmd == "layouts") {
      uint32_t pcap = 0, ccap = 0;
      in >> pcap >> ccap;
      FqWorkLayouts L{};
      const int rc = plan_work_layouts(t, pcap, ccap, B, &L);
      std::cout << rc;
      for (const FqWorkLayout* w : {&L.all, &L.latency}) {
        std::cout << " |";
        for (int c = 0; c < FQ_NCLS; c++) std::cout << ' ' << w->lo[c] << ' ' << w->hi[c] << ' ' << w->off[c] << ' ' << w->cap[c] << " ;";
      }
      std::cout << " | " << L.words << '\n';
    } else {
      uint32_t n = 0, hcap = 0;
      int W = 0, H = 0, path = 0, pf = 0;
      in >> n >> W >> H >> hcap >> path >> pf;
      if (!in) { std::cout << "bad input\n"; return 1; }
      const LaunchPlan p = plan_launch(t, n, W, H, hcap, path, cus, pf != 0);
      std::cout << p.latency << ' ' << p.cc_waves << ' ' << p.border_per_wave << ' ' << p.cc_root_grid << ' ' << p.select_chunks << ' '
                << p.select_grid << ' ' << p.decode_grid << " |";
      auto stream = [](int s) { return s == FIT_MAIN ? std::string("s") : std::to_string(s); };
      for (int i = 0; i < p.nsteps; i++) {
        const FitStep& s = p.steps[i];
        if (s.kind == FIT_FORK) std::cout << " F";
        else if (s.kind == FIT_PREFILTER) std::cout << " P" << p.prefilter_nt << ':' << s.grid << ':' << stream(s.stream);
        else std::cout << " C" << s.cls << (s.compact ? "*" : "") << ':' << s.grid << ':' << s.pop << ':' << stream(s.stream);
      }
      std::cout << '\n';
    }
  }
  return 0;
}
