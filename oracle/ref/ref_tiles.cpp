/* ref_tiles.cpp -- driver around the reference's own tile coding source (TEST INFRASTRUCTURE).
 *
 * oracle/Makefile links this file with the reference's base/src/projectors/tile_coding.cpp, compiled unmodified by path against
 * the stand-in headers shim/grl/projector.h and shim/grl/environment.h, into oracle/_ref/ref_tiles.  The binary is what pins
 * oracle/tile_coding.c (projection, hash sums, the claim table of safe = 1 / 2) in tests/test_oracle_ref_tiles.py, and what
 * tools/record_ref_envs.py records into tests/golden/ref_tiles.npz for the GPU test.  This file restates nothing of the
 * projector: every number it prints comes out of TileCodingProjector::configure / project / reconfigure or out of indices_.
 *
 * Protocol: that of ref_envs.cpp (one command per line, a word and numbers; one answer per line).
 *
 *   tile_configure tilings memory safe D res[D] wrap[...]   -> ok | error ...    a fresh projector, configure(); the wrapping
 *                                                                                vector is whatever follows res (any length)
 *   tile_project x[D]                        -> idx[tilings]                     project(in): claims under safe >= 1
 *   tile_project_variants base[D-1] n v[n]   -> idx[n * tilings]                 project(base, variants): claims under safe = 2
 *   tile_hash x[D]                           -> h[tilings]                       safe >= 1 only: reconfigure(reset), project(in), then
 *                                                                                indices_ at the slots returned: the full hash sums
 *   tile_claims                              -> indices_[memory]
 *   tile_reset                               -> ok                               reconfigure with action = reset
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <grl/projectors/tile_coding.h>

using namespace grl;

double ref_envs_rand() { return 0; }                                      /* the stand-in's RandGen: no projector draws */

struct Tiles : public TileCodingProjector
{
  const int32_t *claims() const { return indices_; }
  int memory() const { return memory_; }
  int tilings() const { return tilings_; }
  int safe() const { return safe_; }
  size_t dims() const { return scaling_.size(); }
};

static Vector take(const std::vector<double> &a, size_t at, size_t n)
{
  Vector v;
  for (size_t i = 0; i < n; ++i) v.push(a.at(at + i));
  return v;
}

static void print(const ProjectionPtr &p, bool first)
{
  const IndexProjection *ip = dynamic_cast<const IndexProjection*>(p.get());
  for (size_t i = 0; i < ip->indices.size(); ++i) printf("%s%zu", (first && !i) ? "" : " ", ip->indices[i]);
}

struct Driver
{
  std::unique_ptr<Tiles> tiles;

  void reset()
  {
    Configuration c;
    c.set("action", "reset");
    tiles->reconfigure(c);
  }

  bool serve(const std::string &cmd, const std::vector<double> &a)
  {
    if (cmd == "tile_configure" && a.size() >= 4 && a[3] >= 0 && a.size() >= 4 + (size_t)a[3])
    {
      size_t D = (size_t)a[3];
      Configuration c;
      c.set("tilings", (int)a[0]);
      c.set("memory", (int)a[1]);
      c.set("safe", (int)a[2]);
      c.set("resolution", take(a, 4, D));
      c.set("wrapping", take(a, 4 + D, a.size() - 4 - D));
      tiles.reset();
      std::unique_ptr<Tiles> fresh(new Tiles());
      fresh->configure(c);
      tiles = std::move(fresh);
      printf("ok");
      return true;
    }
    if (!tiles)
      throw Exception("no projector is configured");
    size_t D = tiles->dims();
    if (cmd == "tile_project" && a.size() == D)
      print(tiles->project(take(a, 0, D)), true);
    else if (cmd == "tile_project_variants" && D >= 1 && a.size() >= D && a.size() == D + (size_t)a[D - 1])
    {
      std::vector<Vector> variants;
      std::vector<ProjectionPtr> out;
      for (size_t i = D; i < a.size(); ++i) variants.push_back(VectorConstructor(a[i]));
      tiles->project(take(a, 0, D - 1), variants, &out);
      for (size_t i = 0; i < out.size(); ++i) print(out[i], i == 0);
    }
    else if (cmd == "tile_hash" && a.size() == D)
    {
      if (!tiles->claims())
        throw Exception("tile_hash needs safe >= 1");
      reset();
      ProjectionPtr p = tiles->project(take(a, 0, D));
      const IndexProjection *ip = dynamic_cast<const IndexProjection*>(p.get());
      for (size_t i = 0; i < ip->indices.size(); ++i) printf("%s%u", i ? " " : "", (unsigned int)tiles->claims()[ip->indices[i]]);
    }
    else if (cmd == "tile_claims" && a.empty())
    {
      if (!tiles->claims())
        throw Exception("tile_claims needs safe >= 1");
      for (int i = 0; i < tiles->memory(); ++i) printf("%s%d", i ? " " : "", (int)tiles->claims()[i]);
    }
    else if (cmd == "tile_reset" && a.empty())
    {
      reset();
      printf("ok");
    }
    else
      return false;
    return true;
  }
};

int main()
{
  Driver driver;
  char *line = NULL;
  size_t cap = 0;
  while (getline(&line, &cap, stdin) > 0)
  {
    std::vector<double> args;
    char *save = NULL, *word = strtok_r(line, " \t\r\n", &save);
    if (!word)
      continue;
    std::string cmd = word;
    bool parsed = true;
    while ((word = strtok_r(NULL, " \t\r\n", &save)))
    {
      char *end = NULL;
      args.push_back(strtod(word, &end));
      parsed = parsed && end != word && *end == 0;
    }
    try
    {
      if (!parsed || !driver.serve(cmd, args))
        printf("error unknown command or wrong argument count: %s", cmd.c_str());
    }
    catch (const Exception &e)
    {
      printf("error %s", e.what().c_str());
    }
    catch (const std::exception &e)
    {
      printf("error %s", e.what());
    }
    printf("\n");
    fflush(stdout);
  }
  free(line);
  return 0;
}
