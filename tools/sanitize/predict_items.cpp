// ASan + UBSan over wrenc_amd/csrc/predict_items.h: the check and the output size of the items of wrenc_gpu_test_predict,
// over the cases of tests/test_predict_layout.py and over random items -- words of any value in every field, and items
// made legal but for one field.  Whatever it is given, the layout must write offsets[0 .. n] and nothing else, and what it
// accepts must fit the picture and the buffers the kernel indexes with it.
// Stand-alone (tools/sanitize/run.sh builds and runs it); no HIP, never loaded into Python.
#include <cstdio>
#include <random>
#include <vector>

#include "../../wrenc_amd/csrc/predict_items.h"

using namespace wrenc;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "predict_items: line %d: %s\n", __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

struct Item {
    int32_t q[5];
};
static int32_t pack(int nc, int m0, int m1 = 0, int m2 = 0) { return (int32_t)((uint32_t)nc << 24 | m2 << 16 | m1 << 8 | m0); }

// what an accepted item promises the kernel: the block lies in the picture on its own grid, and every mode it decodes is
// one the device functions take
static int check_accepted(int W, int H, const int32_t* q, size_t bytes) {
    const int x = q[0], y = q[1], lg = q[2], kind = q[3], mode = q[4], n = 1 << lg;
    CHECK(lg >= 2 && lg <= 5 && x >= 0 && y >= 0 && x + n <= W && y + n <= H && x % n == 0 && y % n == 0 && mode >= 0);
    CHECK(bytes >= 16 && bytes <= 3 * 1024);
    if (kind >= PK_SAD_LUMA && kind <= PK_SAD_BOTH) {
        CHECK((mode & 255) >= 2 && (mode & 255) <= 66 && ((mode >> 8) & 255) >= 1 && ((mode >> 8) & 255) <= 16 && (mode >> 16) >= 1);
    } else if (kind == PK_PACK8 || kind == PK_PACK16) {
        CHECK((mode >> 24) >= 1 && (mode >> 24) <= (kind == PK_PACK8 ? 3 : 2) && lg == (kind == PK_PACK8 ? 3 : 4));
        for (int j = 0; j < (mode >> 24); ++j) CHECK(((mode >> (8 * j)) & 255) <= 66 || ((mode >> (8 * j)) & 255) == 255);
    } else {
        CHECK(kind >= 0 && kind <= PK_FULL_CHROMA && kind != 3 && (mode <= 66 || (mode >= 81 && mode <= 83 && (kind == PK_CHROMA || kind == PK_FULL_CHROMA))));
    }
    return 0;
}

int main() {
    const int W = 64, H = 64;
    const int32_t list = 2 | 1 << 8 | 1 << 16;
    // tests/test_predict_layout.py: one item of every kind at its smallest legal size, and its bytes
    const struct { Item it; size_t bytes; } good[] = {
        {{{0, 0, 2, 0, 0}}, 16}, {{{8, 8, 3, 1, 0}}, 32}, {{{4, 60, 2, 2, 66}}, 16}, {{{0, 0, 2, 4, list}}, 64},
        {{{0, 0, 3, 5, list}}, 64}, {{{0, 0, 3, 6, list}}, 64}, {{{0, 0, 3, 7, 0}}, 64}, {{{0, 0, 3, 8, 0}}, 192},
        {{{0, 0, 3, 9, 81}}, 96}, {{{0, 0, 3, 10, pack(1, 0)}}, 192}, {{{8, 0, 3, 10, pack(3, 0, 255, 66)}}, 576},
        {{{0, 0, 4, 11, pack(1, 50)}}, 1152}, {{{48, 48, 4, 11, pack(2, 255, 1)}}, 2304},
    };
    const Item bad[] = {
        {{4, 0, 3, 0, 0}}, {{0, 12, 4, 0, 0}}, {{64, 0, 3, 0, 0}}, {{0, 64, 2, 0, 0}}, {{-8, 0, 3, 0, 0}}, {{0, 0, 1, 0, 0}},
        {{0, 0, 6, 0, 0}}, {{0, 0, 2, 1, 0}}, {{0, 0, 3, 2, 0}}, {{0, 0, 2, 5, list}}, {{0, 0, 2, 9, 0}}, {{0, 0, 3, 0, 67}},
        {{0, 0, 3, 8, 67}}, {{0, 0, 3, 0, 81}}, {{0, 0, 3, 8, 82}}, {{0, 0, 3, 1, 84}}, {{0, 0, 3, 4, 2 | 0 << 8 | 1 << 16}},
        {{0, 0, 3, 4, 2 | 17 << 8 | 1 << 16}}, {{0, 0, 3, 4, 2 | 1 << 8 | 0 << 16}}, {{0, 0, 3, 4, 2 | 1 << 8 | 65 << 16}},
        {{0, 0, 3, 6, 1 | 1 << 8 | 1 << 16}}, {{0, 0, 3, 6, 67 | 1 << 8 | 1 << 16}}, {{0, 0, 3, 7, 1}}, {{0, 0, 3, 10, pack(0, 0)}},
        {{0, 0, 3, 10, pack(4, 0)}}, {{0, 0, 4, 11, pack(3, 0)}}, {{0, 0, 4, 10, pack(1, 0)}}, {{0, 0, 3, 11, pack(1, 0)}},
        {{0, 0, 3, 10, pack(2, 0, 67)}}, {{0, 0, 4, 11, pack(1, 254)}}, {{0, 0, 3, 0, -1}}, {{0, 0, 3, 10, INT32_MIN | pack(1, 0)}},
        {{0, 0, 3, 3, 0}}, {{0, 0, 3, 12, 0}}, {{0, 0, 31, 0, 0}}, {{0, 0, 32, 0, 0}}, {{0, 0, -1, 0, 0}}, {{INT32_MAX, INT32_MAX, 5, 0, 0}},
    };
    size_t want = 0;
    std::vector<int32_t> all;
    for (const auto& g : good) {
        CHECK(predict_item_bytes(W, H, g.it.q) == g.bytes);
        all.insert(all.end(), g.it.q, g.it.q + 5);
        want += g.bytes;
    }
    {
        const int n = (int)(all.size() / 5);
        std::vector<size_t> at((size_t)n + 1); // exactly what the layout may write
        CHECK(predict_items_layout(W, H, n, all.data(), at.data()) == -1 && at[0] == 0 && at[(size_t)n] == want);
    }
    for (const Item& b : bad) {
        CHECK(predict_item_bytes(W, H, b.q) == 0);
        for (int pos = 0; pos < 3; ++pos) { // first, in the middle, last: refused at its own index
            std::vector<int32_t> three;
            for (int i = 0; i < 3; ++i) three.insert(three.end(), i == pos ? b.q : good[0].it.q, (i == pos ? b.q : good[0].it.q) + 5);
            std::vector<size_t> at(4);
            CHECK(predict_items_layout(W, H, 3, three.data(), at.data()) == pos);
        }
    }
    // random items: any word anywhere; then legal items with one field replaced by any word
    std::mt19937 rng(20260);
    const auto word = [&]() {
        const uint32_t r = rng();
        switch (rng() % 4) {
        case 0: return (int32_t)r;
        case 1: return (int32_t)(r % 128);
        case 2: return (int32_t)(r % 16) - 2;
        default: return (int32_t)((r % 4) << 24 | (r >> 8 & 0xFFFF));
        }
    };
    long accepted = 0;
    for (int round = 0; round < 400000; ++round) {
        const int w = 32 * (1 + (int)(rng() % 4)), h = 32 * (1 + (int)(rng() % 4));
        Item it = good[rng() % (sizeof(good) / sizeof(good[0]))].it;
        if (round & 1)
            it.q[rng() % 5] = word();
        else
            for (int32_t& v : it.q) v = word();
        const size_t bytes = predict_item_bytes(w, h, it.q);
        if (bytes) {
            ++accepted;
            if (check_accepted(w, h, it.q, bytes)) return 1;
        }
        std::vector<size_t> at(2);
        CHECK(predict_items_layout(w, h, 1, it.q, at.data()) == (bytes ? -1 : 0) && (!bytes || at[1] == bytes));
    }
    CHECK(accepted > 10000);
    // the device keeps 32-bit offsets: a call whose output passes 2^31 - 1 bytes is refused at the item that passes it
    {
        const int n = 1 + (int)(((size_t)1 << 31) / 2304);
        std::vector<int32_t> many;
        for (int i = 0; i < n; ++i) many.insert(many.end(), good[12].it.q, good[12].it.q + 5);
        std::vector<size_t> at((size_t)n + 1);
        CHECK(predict_items_layout(W, H, n, many.data(), at.data()) == n - 1);
        CHECK(predict_items_layout(W, H, n - 1, many.data(), at.data()) == -1 && at[(size_t)n - 1] == (size_t)(n - 1) * 2304);
    }
    printf("predict_items: ok (%ld random items accepted)\n", accepted);
    return 0;
}
