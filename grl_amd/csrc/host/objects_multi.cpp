// objects_multi.cpp -- experiment/multi, and the readers of the -Q / -E number files (objects.h).
#include <algorithm>
#include <cmath>
#include <fstream>
#include <sstream>

#include "objects_impl.h"

namespace grlx_host {

// experiment/multi (multi.cpp:36-75): `instances` clones of an experiment running side by side, each
// with the identity "@i" in its output names.  Here the clones are the replicas of ONE device
// context (instance i is seeded seed + i; the reference's clones draw their seeds from the shared
// global stream in instantiation order and then race on it, which no golden file pins).
struct MultiExperiment : OnlineLearningExperiment {
  GRLX_TYPEINFO("experiment/multi")
  int instances = 1;
  OnlineLearningExperiment *prototype = nullptr;
  void request(const std::string &, ConfigurationRequest *config) override
  {
    config->push_back(CRP("instances", "Number of experiments to run in parallel", instances));
    config->push_back(CRP("experiment", "experiment", "Experiment to run", (Configurable *)nullptr));
  }
  void configure(Configuration &config) override
  {
    instances = config["instances"];
    prototype = dynamic_cast<OnlineLearningExperiment *>(config["experiment"].ptr());
    if (instances < 1) throw bad_param("experiment/multi:instances");
    if (!prototype || dynamic_cast<MultiExperiment *>(prototype)) throw Exception(path() + ": experiment must be an experiment/online_learning");
  }
  std::vector<double> run(const RunOptions &opt) override
  {
    if (opt.sweep_repetitions > 0)
      throw Exception(path() + ": a parameter sweep (-p) lays out its own clones; it is not built together with experiment/multi");
    if (!opt.snapshot_save.empty() || !opt.snapshot_load.empty())
      throw Exception(path() + ": a snapshot (-k / -K) is not built together with experiment/multi (use -r for the clones)");
    RunOptions clones = opt;
    clones.replicas = instances * std::max(1, opt.replicas);
    return prototype->run(clones);
  }
};
GRLX_REGISTER(MultiExperiment)

namespace {
// rows of whitespace-separated finite numbers, `#` comments, every row as long as the first: flag = "-Q" / "-E", what = "observation" / "state"
void read_number_file(const std::string &flag, const std::string &file, const std::string &what, std::vector<double> *out, int *rows, int *cols)
{
  std::ifstream f(file);
  if (!f) throw Exception(flag + ": could not open the " + what + " file '" + file + "'");
  std::string line;
  int line_no = 0;
  out->clear();
  *rows = *cols = 0;
  while (std::getline(f, line))
  {
    line_no++;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    std::istringstream in(line);
    std::string tok;
    int n = 0;
    while (in >> tok)
    {
      char *stop = nullptr;
      const double v = strtod(tok.c_str(), &stop);
      if (*stop != 0 || !std::isfinite(v))
        throw Exception(flag + " " + file + ": line " + std::to_string(line_no) + ": '" + tok + "' is not a finite number");
      out->push_back(v);
      n++;
    }
    if (n == 0) continue;
    if (*rows > 0 && n != *cols)
      throw Exception(flag + " " + file + ": line " + std::to_string(line_no) + " has " + std::to_string(n) + " columns, the lines before it " +
                      std::to_string(*cols));
    *cols = n;
    (*rows)++;
  }
  if (*rows == 0) throw Exception(flag + " " + file + ": no " + what + "s");
}
} // namespace

void read_query_file(RunOptions *opt) { read_number_file("-Q", opt->query_file, "observation", &opt->query_obs, &opt->query_rows, &opt->query_cols); }
void read_evaluate_file(RunOptions *opt)
{
  read_number_file("-E", opt->evaluate_file, "state", &opt->evaluate_states, &opt->evaluate_rows, &opt->evaluate_cols);
}
} // namespace grlx_host
