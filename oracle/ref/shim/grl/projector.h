/* grl/projector.h -- STAND-IN for the reference's header of that name (TEST INFRASTRUCTURE).
 *
 * oracle/Makefile compiles the reference's base/src/projectors/tile_coding.cpp UNMODIFIED, by path, into oracle/_ref/ref_tiles;
 * its own header (grl/projectors/tile_coding.h: the hash, the claim table) comes from the reference's include directory.  This file
 * takes the place of the framework header that one asks for.  It is our own text: Vector, Configuration and the exceptions are
 * those of the stand-in grl/environment.h beside it, and the names below are here because the compiler asks for them.  The
 * quantisation, the displacement, the wrapping, the hash and the claim walk are the reference's; the one thing here that computes
 * a number is safe_mod, whose home in the reference (grl/utils.h) cannot be included without the vector algebra.
 */
#ifndef GRL_ORACLE_REF_SHIM_PROJECTOR_H_
#define GRL_ORACLE_REF_SHIM_PROJECTOR_H_

#include <memory>
#include <sstream>

#include <grl/environment.h>

/* the sources' log lines: built (they stream Vectors) and dropped */
#define ERROR(m) do { std::ostringstream grl_log_; grl_log_ << m; } while (0)
#define WARNING(m) do { std::ostringstream grl_log_; grl_log_ << m; } while (0)

namespace grl
{

template<class T> bool safe_delete_array(T **obj)
{
  bool had = *obj != NULL;
  delete[] *obj;
  *obj = NULL;
  return had;
}

/* C's remainder lifted into [0, Y): the reference's grl/utils.h has it, and that header needs the rest of the framework */
template<class I> inline I safe_mod(I X, I Y)
{
  I r = X % Y;
  return r < 0 ? r + Y : r;
}

struct Projection
{
  virtual ~Projection() { }
};
struct IndexProjection : Projection
{
  std::vector<size_t> indices;
};
using ProjectionPtr = std::shared_ptr<Projection>;

struct Projector : Configurable
{
  enum ProjectionLifetime { plIndefinite, plWrite, plUpdate };
  virtual ProjectionPtr project(const Vector &input) const = 0;
  virtual void project(const Vector &input, const std::vector<Vector> &variants, std::vector<ProjectionPtr> *projections) const = 0;
};

}

#endif
