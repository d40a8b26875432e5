// objects_csv.cpp -- exporter/csv (exporters/csv.cpp:37-206, exporter.h:62-95) and the two transition logs an
// experiment/online_learning writes through it from the device's taps.
#include <algorithm>
#include <iomanip>
#include <sstream>

#include "objects_impl.h"

namespace grlx_host {

void CSVExporter::request(const std::string &, ConfigurationRequest *config)
{
  config->push_back(CRP("file", "Output base filename", file));
  config->push_back(CRP("fields", "Comma-separated list of fields to write", fields));
  config->push_back(CRP("style", "Header style", style));
  config->push_back(CRP("variant", "Variant to export", variant));
  config->push_back(CRP("enabled", "Enable writing to output file", enabled, CRP::Online));
  config->push_back(CRP("offset", "Start of numbering", offset));
}
void CSVExporter::configure(Configuration &config)
{
  file = config["file"].str(); fields = config["fields"].str(); style = config["style"].str(); variant = config["variant"].str();
  enabled = config["enabled"]; offset = config["offset"];
  if (file.empty()) throw bad_param("exporter/csv:file");
  if (style != "none" && style != "line" && style != "meshup") throw bad_param("exporter/csv:style");
  if (variant != "test" && variant != "learn" && variant != "all") throw bad_param("exporter/csv:variant");
  if (enabled != 0 && enabled != 1) throw bad_param("exporter/csv:enabled");
}
// csv.cpp:66-121
void CSVExporter::init(const std::vector<std::string> &h)
{
  headers = h;
  order.clear();
  if (fields.empty())
  {
    for (size_t i = 0; i < h.size(); ++i) order.push_back(i);
    return;
  }
  std::stringstream list(fields);
  std::string item;
  while (std::getline(list, item, ','))
  {
    item.erase(std::remove_if(item.begin(), item.end(), [](char ch) { return ch == ' ' || ch == '\t'; }), item.end());
    bool known = false;
    for (size_t i = 0; i < h.size(); ++i)
      if (h[i] == item) { order.push_back(i); known = true; }
    if (!known)
    {
      log(0, "Requested unregistered field '" + item + "'");
      throw bad_param("exporter/csv:fields");
    }
  }
}
// csv.cpp:123-157
void CSVExporter::open(const std::string &which, bool append)
{
  if (stream.is_open()) stream.close();
  if (variant != "all" && variant != which) return;
  std::string name = which.empty() ? file : file + "-" + which;
  int &runs_seen = counter[name];
  if (runs_seen == 0) runs_seen = offset;
  if (!append) runs_seen++;
  name += "-" + std::to_string(runs_seen - 1) + ".csv";
  std::ifstream probe(name, std::ios::binary | std::ios::ate);
  header_due = !append || !probe || probe.tellg() == std::streampos(0);
  probe.close();
  stream.open(name, append ? (std::ios::out | std::ios::app) : (std::ios::out | std::ios::trunc));
  if (!stream.good())
  {
    log(0, "Could not open '" + name + "' for writing");
    throw bad_param("exporter/csv:file");
  }
}
// csv.cpp:159-206
void CSVExporter::write(const std::vector<std::vector<double>> &vars)
{
  if (!enabled || !stream.is_open()) return;
  if (vars.size() != headers.size()) { log(0, "Variable list does not match header list"); return; }
  if (header_due && style != "none")
  {
    const bool mesh = style == "meshup";
    if (mesh) stream << "COLUMNS:" << std::endl;
    for (size_t i = 0; i < order.size(); ++i)
      for (size_t k = 0; k < vars[order[i]].size(); ++k)
      {
        stream << headers[order[i]] << "[" << k << "]";
        if (i + 1 < order.size() || k + 1 < vars[order[i]].size()) stream << ", ";
        if (mesh) stream << std::endl;
      }
    if (mesh) stream << "DATA:" << std::endl;
    else stream << std::endl;
  }
  header_due = false;
  for (size_t i = 0; i < order.size(); ++i)
    for (size_t k = 0; k < vars[order[i]].size(); ++k)
    {
      stream << std::fixed << std::setw(11) << std::setprecision(6) << vars[order[i]][k];
      if (i + 1 < order.size() || k + 1 < vars[order[i]].size()) stream << ", ";
    }
  stream << std::endl;
}
GRLX_REGISTER(CSVExporter)

// ModeledEnvironment's own log (modeled.cpp:156-157, 200-203): one row per step with the state the step started
// from and the environment's cumulative learn / test time BEFORE the step; a numbered file per variant is
// started by the first episode of that variant, later episodes append
void write_environment_log(CSVExporter *out, const std::vector<grlx_tap> &taps, int state_dims, int obs_dims, double control_step)
{
  double time_learn = 0, time_test = 0;
  std::vector<double> before((size_t)state_dims, 0.);
  bool is_test = false;
  for (size_t k = 0; k < taps.size(); ++k)
  {
    const grlx_tap &tp = taps[k];
    if (tp.terminal == -1)
    {
      is_test = tp.test != 0;
      out->open(is_test ? "test" : "learn", (is_test ? time_test : time_learn) != 0.0);
    }
    else
    {
      double &time = is_test ? time_test : time_learn;
      const std::vector<double> obs(tp.obs, tp.obs + obs_dims);
      // the action of this row is the one the step was taken with: the previous record's
      out->write({{time}, before, obs, {taps[k - 1].action}, {tp.reward}, {(double)tp.terminal}});
      time += control_step;                          // model tau = control_step (modeled.cpp:176, 203)
    }
    before.assign(tp.state, tp.state + state_dims);
  }
  out->close();
}

// online_learning.cpp:127-131 (new numbered files per run), :164-165 (append per trial), :183-206 (rows)
void write_experiment_log(CSVExporter *out, const std::vector<grlx_tap> &taps, int obs_dims)
{
  out->open("test", false);
  out->open("learn", false);
  double total_time = 0, applied = 0;
  for (const grlx_tap &tp : taps)
  {
    const std::vector<double> obs(tp.obs, tp.obs + obs_dims);
    if (tp.terminal == -1)
    { // start of a trial: first observation, first action
      out->open(tp.test ? "test" : "learn", true);
      total_time = 0;
      out->write({{total_time}, obs, {tp.action}, {0.}, {0.}});
    }
    else
    { // a step: the action that was applied, the observation and reward it led to
      total_time += 1;                          // tau = 1 (discrete_time)
      out->write({{total_time}, obs, {applied}, {tp.reward}, {(double)tp.terminal}});
    }
    applied = tp.action;
  }
  out->close();
}

} // namespace grlx_host
