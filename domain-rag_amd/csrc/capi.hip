// capi.hip — version / error plumbing of the C ABI (include/domainrag_hip.h).
#include "drag_common.h"
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static thread_local char g_err[1024] = "";

void drag_set_error(const char* msg) {
  strncpy(g_err, msg ? msg : "unknown error", sizeof(g_err) - 1);
  g_err[sizeof(g_err) - 1] = 0;
}

extern "C" const char* drag_last_error(void) { return g_err; }
extern "C" int drag_version(void) { return 100; }  // 0.1.0
extern "C" int drag_experiments_built(void) { return DRAG_EXP; }

// ---- tuning switches (measurement only: every setting computes the same values unless its comment says otherwise).  Everything here is
// generated from DRAG_OPTIONS (drag_common.h).  Initial values come from the environment ONCE — $DRAG_<NAME IN UPPER CASE>: unset = the
// table's default, set but empty = 1, else atoi — and drag_set_option changes them at run time so one process can A/B kernels.
struct OptRow { const char* name; int def; int exp; };
#define DRAG_OPT_ROW(id, name, def, exp) {name, def, exp},
static const OptRow g_opt_rows[DRAG_OPT_COUNT] = {DRAG_OPTIONS(DRAG_OPT_ROW)};
#undef DRAG_OPT_ROW
static int g_opt[DRAG_OPT_COUNT];
static bool g_opt_init = false;

// does `value` of switch i exist only in a DRAG_EXPERIMENTS library?
static bool opt_is_experiment(int i, int value) {
  const int exp = g_opt_rows[i].exp;
  return exp == DRAG_OPT_EXP_ANY ? value != 0 : (exp != DRAG_OPT_PRODUCT && value == exp);
}

static void opt_init() {
  if (g_opt_init) return;
  for (int i = 0; i < DRAG_OPT_COUNT; ++i) {
    char env[64] = "DRAG_";
    size_t n = strlen(env);
    for (const char* c = g_opt_rows[i].name; *c && n + 1 < sizeof(env); ++c) env[n++] = (char)toupper((unsigned char)*c);
    env[n] = 0;
    const char* e = getenv(env);
    g_opt[i] = e ? (*e ? atoi(e) : 1) : g_opt_rows[i].def;
    // the product library has no experiment kernels: their environment switches are ignored
    if (!DRAG_EXP && opt_is_experiment(i, g_opt[i])) g_opt[i] = g_opt_rows[i].def;
  }
  g_opt_init = true;
}

int drag_opt(int idx) {
  opt_init();
  return g_opt[idx];
}

static int opt_find(const char* name, const char* who) {
  for (int i = 0; i < DRAG_OPT_COUNT; ++i)
    if (strcmp(name, g_opt_rows[i].name) == 0) return i;
  char msg[sizeof(g_err)];
  size_t n = (size_t)snprintf(msg, sizeof(msg), "%s: unknown option (", who);
  for (int i = 0; i < DRAG_OPT_COUNT && n < sizeof(msg); ++i)
    n += (size_t)snprintf(msg + n, sizeof(msg) - n, "%s%s", i ? ", " : "", g_opt_rows[i].name);
  if (n < sizeof(msg)) snprintf(msg + n, sizeof(msg) - n, ")");
  drag_set_error(msg);
  return -1;
}

extern "C" int drag_set_option(const char* name, int32_t value) {
  DRAG_CHECK(name != nullptr, "drag_set_option: null name");
  opt_init();
  const int i = opt_find(name, "drag_set_option");
  if (i < 0) return -1;
  if (!DRAG_EXP && opt_is_experiment(i, value)) {
    char msg[160];
    snprintf(msg, sizeof(msg), "drag_set_option: %s = %d is one of the experiments (measured non-improvements): build the library with DRAG_EXPERIMENTS=1",
             name, (int)value);
    drag_set_error(msg);
    return -1;
  }
  g_opt[i] = value;
  return 0;
}

extern "C" int drag_get_option(const char* name, int32_t* value) {
  DRAG_CHECK(name != nullptr && value != nullptr, "drag_get_option: null argument");
  opt_init();
  const int i = opt_find(name, "drag_get_option");
  if (i < 0) return -1;
  *value = g_opt[i];
  return 0;
}

extern "C" const char* drag_option_name(int32_t index) { return index >= 0 && index < DRAG_OPT_COUNT ? g_opt_rows[index].name : nullptr; }
