// tf_rule_probe.cpp — a C face for csrc/opv_tf_rule.h, built with g++ by tests/test_tf_clamp_rule_host.py.
#include <stdint.h>

#include "opv_tf_rule.h"

extern "C" {
int probe_tf_clamp_cannot_act(double tf, uint64_t n) { return opv_tf_clamp_cannot_act(tf, n) ? 1 : 0; }
double probe_tf_beta(void) { return kOpvTfBeta; }
double probe_tf_max(void) { return kOpvTfMax; }
// A worst case, iterated in the kernel's own arithmetic: n / 39 + 2 symbols with the same timing error `ted` each (the rule covers
// |ted| <= 2), tf = fma(beta, ted, tf) and no clamp. Returns the largest |tf| seen, the start included.
double probe_tf_worst_walk(double tf, uint64_t n, double ted) {
    double worst = tf < 0 ? -tf : tf;
    for (uint64_t k = n / 39u + 2u; k != 0; --k) {
        tf = __builtin_fma(kOpvTfBeta, ted, tf);
        const double a = tf < 0 ? -tf : tf;
        if (a > worst) worst = a;
    }
    return worst;
}
}
