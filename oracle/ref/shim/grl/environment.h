/* grl/environment.h -- STAND-IN for the reference's header of that name (TEST INFRASTRUCTURE).
 *
 * oracle/Makefile compiles five of the reference's environment sources UNMODIFIED, by path, into oracle/_ref/ref_envs:
 *   base/src/environments/acrobot.cpp, cart_pole.cpp, pendulum.cpp, compass_walker/SWModel.cpp and compass_walker/compass_walker.cpp
 * (and, through the stand-in grl/projector.h beside this file, base/src/projectors/tile_coding.cpp into oracle/_ref/ref_tiles).
 * Their own headers (acrobot.h, cart_pole.h, pendulum.h, SWModel.h, compass_walker.h, tile_coding.h) come from the reference's
 * include directory; this file takes the place of the framework header they all ask for, which needs Eigen and the configuration
 * machinery.  It is our own text, written from what the compiler asks for when it compiles those files: every name below is here
 * because one of them uses it, and does the least that lets the code under test (eom, start, observe, evaluate, step, singleStep,
 * configure, _project) run as written.  Nothing here computes a number the tests compare, except Vector's element access and
 * `extend` (a concatenation).
 */
#ifndef GRL_ORACLE_REF_SHIM_ENVIRONMENT_H_
#define GRL_ORACLE_REF_SHIM_ENVIRONMENT_H_

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <deque>
#include <initializer_list>
#include <iostream>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

/* supplied by the driver: the next draw of the thread-local generator (the caller of the driver hands the draws over) */
double ref_envs_rand();

#define TYPEINFO(type, description)
#define REGISTER_CONFIGURABLE(cls)

namespace grl
{

/* a vector of doubles: size, resize, element access, and `(v.array() != 0).count()` */
class Vector
{
  public:
    struct Mask
    {
      long n;
      long count() const { return n; }
    };
    struct Elements
    {
      const std::vector<double> *d;
      Mask operator!=(double x) const
      {
        Mask m = {0};
        for (size_t i = 0; i < d->size(); ++i) m.n += (*d)[i] != x;
        return m;
      }
    };

    Vector() { }
    explicit Vector(size_t n) : d_(n) { }
    size_t size() const { return d_.size(); }
    void resize(size_t n) { d_.resize(n); }
    double &operator[](size_t i) { return d_.at(i); }
    const double &operator[](size_t i) const { return d_.at(i); }
    Elements array() const { Elements e = {&d_}; return e; }
    void push(double x) { d_.push_back(x); }

  private:
    std::vector<double> d_;
};

inline std::ostream &operator<<(std::ostream &os, const Vector &v)
{
  for (size_t i = 0; i < v.size(); ++i) os << (i ? " " : "") << v[i];
  return os;
}
inline Vector extend(const Vector &head, const Vector &tail)
{
  Vector v = head;
  for (size_t i = 0; i < tail.size(); ++i) v.push(tail[i]);
  return v;
}

inline void fill_vector(Vector *) { }
template<class T, class... Rest> void fill_vector(Vector *v, T first, Rest... rest)
{
  v->push((double)first);
  fill_vector(v, rest...);
}
template<class... Args> Vector VectorConstructor(Args... args)
{
  Vector v;
  fill_vector(&v, args...);
  return v;
}
inline Vector ConstantVector(size_t n, double x)
{
  Vector v;
  for (size_t i = 0; i < n; ++i) v.push(x);
  return v;
}

struct Observation
{
  Vector v;
  bool absorbing;
  Observation() : absorbing(false) { }
  operator Vector() const { return v; }
  size_t size() const { return v.size(); }
  double &operator[](size_t i) { return v[i]; }
  const double &operator[](size_t i) const { return v[i]; }
};

/* what rewardHessian returns: never looked at */
struct Matrix
{
  static Matrix Identity(size_t, size_t) { return Matrix(); }
};
inline Matrix diagonal(const Vector &) { return Matrix(); }

struct Action
{
  Vector v;
  size_t size() const { return v.size(); }
  double &operator[](size_t i) { return v[i]; }
  const double &operator[](size_t i) const { return v[i]; }
};

class Exception
{
  public:
    Exception(const std::string &what) : what_(what) { }
    const std::string &what() const { return what_; }
  private:
    std::string what_;
};
class bad_param : public Exception
{
  public:
    bad_param(const std::string &which) : Exception("bad parameter " + which) { }
};

struct RandGen
{
  static double get() { return ref_envs_rand(); }
};

inline double normalize_angle(double a) { return a - 2*M_PI*std::floor((a + M_PI)/(2*M_PI)); }  /* regulator task only: not driven */

class Exporter
{
  public:
    void init(std::initializer_list<std::string>) { }
    void open(const std::string &, bool) { }
    void write(std::initializer_list<Vector>) { }
};

/* a requested parameter: the sources describe theirs in many shapes, none of which the driver reads */
struct CRP
{
  enum Mutability { Configuration, System, Online };
  template<class... Args> CRP(const Args &...) { }
};
struct ConfigurationRequest
{
  void push_back(const CRP &) { }
};

/* one value of a Configuration: converts to whatever the member it is assigned to holds */
struct ConfigurationValue
{
  double scalar;
  Vector vector;
  std::string string;
  ConfigurationValue() : scalar(0) { }
  const std::string &str() const { return string; }
  template<class T> operator T() const { return (T)scalar; }
  Vector v() const { return vector; }
  void *ptr() const { return NULL; }
};
class Configuration
{
  public:
    ConfigurationValue &operator[](const std::string &key) { return values_[key]; }
    ConfigurationValue operator[](const std::string &key) const { return has(key) ? values_.find(key)->second : ConfigurationValue(); }
    bool has(const std::string &key) const { return values_.count(key) != 0; }
    template<class T> bool get(const std::string &key, T &x) const
    {
      if (has(key)) x = (T)values_.find(key)->second.scalar;
      return has(key);
    }
    void set(const std::string &key, const Vector &v) { values_[key].vector = v; }
    void set(const std::string &key, const char *text) { values_[key].string = text; }
    template<class T> void set(const std::string &key, T x) { values_[key].scalar = (double)x; }
  private:
    std::map<std::string, ConfigurationValue> values_;
};

class Configurable
{
  public:
    virtual ~Configurable() { }
    virtual void request(ConfigurationRequest *) { }
    virtual void configure(Configuration &) { }
    virtual void reconfigure(const Configuration &) { }
    virtual Configurable &copy(const Configurable &) { return *this; }
};
class Dynamics : public Configurable
{
  public:
    virtual void eom(const Vector &state, const Vector &actuation, Vector *xd) const = 0;
};
class Model : public Configurable
{
  public:
    virtual double step(const Vector &state, const Vector &actuation, Vector *next) const = 0;
};
class Sandbox : public Configurable
{
  public:
    virtual void start(const Vector &hint, Vector *state) = 0;
    virtual double step(const Vector &actuation, Vector *next) = 0;
  protected:
    Vector state_;
};
class Task : public Configurable
{
  public:
    virtual void start(int test, Vector *state) = 0;
    virtual void observe(const Vector &state, Observation *obs, int *terminal) const = 0;
    virtual void evaluate(const Vector &state, const Action &action, const Vector &next, double *reward) const = 0;
};
/* the acrobot's quadratic-cost task derives from this; the driver never makes one */
class RegulatorTask : public Task
{
  public:
    virtual void start(int, Vector *) { }
    virtual void observe(const Vector &, Observation *, int *) const { }
    virtual void evaluate(const Vector &, const Action &, const Vector &, double *) const { }
  protected:
    Vector start_, goal_, stddev_, q_, r_;
    double timeout_;
};

}

#endif
