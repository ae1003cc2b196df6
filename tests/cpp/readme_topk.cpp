// The snippet of README.md, "The k largest", compiled and run by tests/test_topk_cpp.py so it cannot rot, with data for which the
// answer is known.
#include <sm.h>

#include <cstdint>
#include <cstdio>
#include <vector>

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) ++g_failures, std::printf("FAIL line %d  %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    auto logits = sm::ones<float>(512, 1000);                     // one row per sample
    for (std::size_t i = 0; i < 512; ++i) logits.data[i * 1000 + (i * 7) % 1000] = 3.0f, logits.data[i * 1000 + (i * 7 + 1) % 1000] = 2.0f;

    auto [scores, classes] = sm::topk(logits, 5);                 // shape {512, 5} each: the five best of each row, best first
    auto mask = sm::zeros<float>(512, 1000);
    mask.put_along_axis(classes, 1.0f, -1, sm::index_mode::checked, /*unique=*/true);  // 1 at the top-5 classes of each row
    auto picked = sm::take_along_axis(logits, classes, -1);       // the positions pick the scores back
    auto margin = scores(SLICE_ALL, SLICE(0, 1)) - scores(SLICE_ALL, SLICE(1, 2));  // ... and the scores feed the next chain
    auto [lowest, where] = logits.topk(3, 0, /*largest=*/false);  // member form: the three smallest of each column

    CHECK((scores.shape() == std::vector<std::size_t>{512, 5}) && classes.shape() == scores.shape());
    int bad = 0;
    for (std::size_t i = 0; i < 512; ++i) {
        const std::int64_t best = static_cast<std::int64_t>((i * 7) % 1000), second = static_cast<std::int64_t>((i * 7 + 1) % 1000);
        bad += classes(i, 0) != best || classes(i, 1) != second || scores(i, 0) != 3.0f || scores(i, 1) != 2.0f || scores(i, 4) != 1.0f;
        bad += classes(i, 2) != (best == 0 || second == 0 ? (best == 1 || second == 1 ? 2 : 1) : 0);  // then the ties, in rising position
        float sum = 0.0f;
        for (std::size_t j = 0; j < 1000; ++j) sum += mask.cdata()[i * 1000 + j];
        bad += sum != 5.0f || mask.cdata()[i * 1000 + static_cast<std::size_t>(best)] != 1.0f;
        bad += margin.cdata()[i] != 1.0f;
        for (std::size_t j = 0; j < 5; ++j) bad += picked.cdata()[i * 5 + j] != scores.cdata()[i * 5 + j];
    }
    CHECK(bad == 0);
    CHECK((lowest.shape() == std::vector<std::size_t>{3, 1000}) && lowest.cdata()[0] == 1.0f && where.totalSize == 3000);
    std::printf("readme_topk: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
