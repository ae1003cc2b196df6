// The snippet of README.md, "Softmax, log-softmax and logsumexp", compiled and run by tests/test_softmax_cpp.py so it cannot rot,
// with data for which the answer is known.
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) ++g_failures, std::printf("FAIL line %d  %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    auto logits = sm::ones<float>(512, 1000);                       // one row per sample
    auto labels = sm::zeros<std::int64_t>(512, 1);                  // the true class of each sample
    for (std::size_t i = 0; i < 512; ++i) logits.data[i * 1000 + (i * 7) % 1000] = 3.0f, labels.data[i] = static_cast<std::int64_t>((i * 7) % 1000);

    auto probs = sm::softmax(logits);                               // shape {512, 1000}: every row sums to 1
    auto predicted = sm::argmax(probs, -1);                         // ... and feeds argmax, never leaving HBM
    auto logp = sm::log_softmax(logits);                            // (x - max) - log(sum(exp(x - max))): small probabilities keep their logarithm
    auto picked = sm::take_along_axis(logp, labels, -1);            // shape {512, 1}: the log-probability of the true class
    double cross_entropy = -picked.sum() / 512.0;                   // the mean negative log-likelihood
    auto per_class = logits.logsumexp(0);                           // member form, over the columns: shape {1000}

    // a row is 999 ones and one 3: the true class has probability e^2 / (e^2 + 999)
    const double best = std::exp(2.0) / (std::exp(2.0) + 999.0), other = 1.0 / (std::exp(2.0) + 999.0);
    CHECK((probs.shape() == std::vector<std::size_t>{512, 1000}) && (picked.shape() == std::vector<std::size_t>{512, 1}) && (per_class.shape() == std::vector<std::size_t>{1000}));
    int bad = 0;
    for (std::size_t i = 0; i < 512; ++i) {
        const std::size_t c = (i * 7) % 1000;
        bad += predicted.cdata()[i] != static_cast<std::int64_t>(c);
        bad += !(std::fabs(probs.cdata()[i * 1000 + c] - best) <= 1e-6 * best) || !(std::fabs(probs.cdata()[i * 1000 + (c + 1) % 1000] - other) <= 1e-6 * other);
        bad += !(std::fabs(picked.cdata()[i] - std::log(best)) <= 1e-6);
    }
    CHECK(bad == 0);
    CHECK(std::fabs(cross_entropy + std::log(best)) <= 1e-6);
    for (std::size_t j = 0; j < 1000; ++j) {  // a column: 512 ones, a few of them raised to 3
        int threes = 0;
        for (std::size_t i = 0; i < 512; ++i) threes += (i * 7) % 1000 == j;
        const double want = std::log((512 - threes) * std::exp(1.0) + threes * std::exp(3.0));
        bad += !(std::fabs(per_class.cdata()[j] - want) <= 1e-6 * want);
    }
    CHECK(bad == 0);
    std::printf("readme_softmax: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
