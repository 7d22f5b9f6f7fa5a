// Stand-alone: the weighted entry points of the host substrate on malformed inputs, compiled together with loader.cpp under
// -fsanitize=address,undefined (tests/test_weights_loader.py builds and runs it).  argv[1] = a scratch directory.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gmsx.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static std::string write_file(const std::string &dir, const char *name, const void *data, size_t bytes) {
    const std::string p = dir + "/" + name;
    std::FILE *f = std::fopen(p.c_str(), "wb");
    if (!f) std::exit(3);
    if (bytes) std::fwrite(data, 1, bytes, f);
    std::fclose(f);
    return p;
}
static std::string write_text(const std::string &dir, const char *name, const std::string &text) { return write_file(dir, name, text.data(), text.size()); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    gmsx_csr *g = nullptr;

    // a good graph, saved as .wsg and read back
    const int32_t src[] = {0, 1, 2, 0, 3, 3}, dst[] = {1, 2, 0, 1, 3, 4}, w[] = {5, 6, 7, 2, 9, 4};
    CHECK(gmsx_csr_from_weighted_edges(-1, 6, src, dst, w, 1, GMSX_RELABEL_NEVER, &g) == GMSX_OK);
    CHECK(gmsx_csr_num_nodes(g) == 5 && gmsx_csr_num_edges_directed(g) == 8 && gmsx_csr_weights(g) != nullptr);
    CHECK(gmsx_csr_weights(g)[0] == 2);  // 0 - 1 twice: the smaller weight
    const std::string good = dir + "/good.wsg";
    CHECK(gmsx_csr_save_wsg(g, good.c_str()) == GMSX_OK);
    const uint64_t f0 = gmsx_csr_fingerprint(g, 0), f1 = gmsx_csr_fingerprint(g, 1), f2 = gmsx_csr_fingerprint(g, 2);
    gmsx_csr *back = nullptr;
    CHECK(gmsx_csr_load_weighted(good.c_str(), 1, GMSX_RELABEL_NEVER, &back) == GMSX_OK);
    CHECK(back && gmsx_csr_fingerprint(back, 0) == f0 && gmsx_csr_fingerprint(back, 1) == f1 && gmsx_csr_fingerprint(back, 2) == f2 && f2 != 0);
    gmsx_csr_free(back);
    gmsx_csr *rel = nullptr;
    CHECK(gmsx_csr_relabel_by_degree(g, &rel) == GMSX_OK && gmsx_csr_weights(rel) != nullptr);
    gmsx_csr_free(rel);

    // truncated .wsg at every length, and headers that announce more than the file holds
    std::vector<unsigned char> bytes;
    {
        std::FILE *f = std::fopen(good.c_str(), "rb");
        if (!f) return 3;
        int c;
        while ((c = std::fgetc(f)) != EOF) bytes.push_back((unsigned char)c);
        std::fclose(f);
    }
    for (size_t cut = 0; cut < bytes.size(); ++cut) {
        const std::string p = write_file(dir, "cut.wsg", bytes.data(), cut);
        gmsx_csr *t = nullptr;
        CHECK(gmsx_csr_load_weighted(p.c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_FORMAT && t == nullptr);
    }
    {
        std::vector<unsigned char> planted(bytes);
        const int64_t huge = int64_t(1) << 40;
        for (int i = 0; i < 8; ++i) planted[1 + i] = (unsigned char)(huge >> (8 * i));  // nnz
        const std::string p = write_file(dir, "planted.wsg", planted.data(), planted.size());
        gmsx_csr *t = nullptr;
        CHECK(gmsx_csr_load_weighted(p.c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_FORMAT);
        planted = bytes;
        planted[17 + 8] = 0xff;  // offsets[1]: not monotone / beyond nnz
        planted[17 + 8 + 6] = 0x7f;
        const std::string q = write_file(dir, "planted2.wsg", planted.data(), planted.size());
        CHECK(gmsx_csr_load_weighted(q.c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_FORMAT);
        planted = bytes;
        planted[bytes.size() - 8 + 3] = 0x7f;  // the last id: out of range
        const std::string r = write_file(dir, "planted3.wsg", planted.data(), planted.size());
        CHECK(gmsx_csr_load_weighted(r.c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_FORMAT);
    }

    // .wel: a missing third column ends the list in front of it; a negative weight is loaded as it is; a huge one is refused; an empty file
    {
        gmsx_csr *t = nullptr;
        CHECK(gmsx_csr_load_weighted(write_text(dir, "short.wel", "0 1 5\n1 2 6\n2 3\n").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_OK);
        CHECK(t && gmsx_csr_num_nodes(t) == 3 && gmsx_csr_num_edges_directed(t) == 4);
        gmsx_csr_free(t);
        t = nullptr;
        CHECK(gmsx_csr_load_weighted(write_text(dir, "neg.wel", "0 1 -5\n1 2 6\n").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_OK);
        CHECK(t && gmsx_csr_weights(t)[0] == -5);
        gmsx_csr_free(t);
        t = nullptr;
        CHECK(gmsx_csr_load_weighted(write_text(dir, "huge.wel", "0 1 4294967296\n").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_OVERFLOW && !t);
        CHECK(gmsx_csr_load_weighted(write_text(dir, "hugeid.wel", "0 4294967296 1\n").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_OVERFLOW && !t);
        CHECK(gmsx_csr_load_weighted(write_text(dir, "empty.wel", "").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_OK);
        CHECK(t && gmsx_csr_num_nodes(t) == 1 && gmsx_csr_num_edges_directed(t) == 0 && gmsx_csr_weights(t) != nullptr);
        CHECK(gmsx_csr_save_wsg(t, (dir + "/empty.wsg").c_str()) == GMSX_OK);
        gmsx_csr_free(t);
        t = nullptr;
        CHECK(gmsx_csr_load_weighted((dir + "/empty.wsg").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_OK);
        gmsx_csr_free(t);
        t = nullptr;
        CHECK(gmsx_csr_load_weighted((dir + "/no_such_file.wel").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_IO);
        CHECK(gmsx_csr_load_weighted((dir + "/x.sg").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_FORMAT);
        CHECK(gmsx_csr_load_weighted(write_text(dir, "bad.gr", "a 1 2\n").c_str(), 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_FORMAT);
    }

    // from_weighted_edges: ids out of range, NULL arrays, no weights
    {
        gmsx_csr *t = nullptr;
        const int32_t bs[] = {0, 7}, bd[] = {1, 2}, bw[] = {1, 1}, ns[] = {0, -1};
        CHECK(gmsx_csr_from_weighted_edges(4, 2, bs, bd, bw, 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_INVALID && !t);
        CHECK(gmsx_csr_from_weighted_edges(-1, 2, ns, bd, bw, 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_INVALID && !t);
        CHECK(gmsx_csr_from_weighted_edges(-1, 2, nullptr, bd, bw, 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_INVALID);
        CHECK(gmsx_csr_from_weighted_edges(-1, -1, bs, bd, bw, 1, GMSX_RELABEL_NEVER, &t) == GMSX_ERR_INVALID);
        CHECK(gmsx_csr_from_weighted_edges(-1, 2, bs, bd, nullptr, 1, GMSX_RELABEL_ALWAYS, &t) == GMSX_OK);
        CHECK(t && gmsx_csr_weights(t) && gmsx_csr_weights(t)[0] >= 1 && gmsx_csr_weights(t)[0] <= 255);
        gmsx_csr_free(t);
        t = nullptr;
        CHECK(gmsx_csr_from_weighted_edges(-1, 0, nullptr, nullptr, nullptr, 1, GMSX_RELABEL_NEVER, &t) == GMSX_OK);
        gmsx_csr_free(t);
        t = nullptr;
        const int64_t off[] = {0, 1, 2};
        const int32_t ng[] = {1, 0}, wg[] = {3, 3};
        CHECK(gmsx_csr_from_arrays_weighted(2, off, ng, nullptr, &t) == GMSX_ERR_INVALID);
        CHECK(gmsx_csr_from_arrays_weighted(2, off, ng, wg, &t) == GMSX_OK && gmsx_csr_weights(t)[1] == 3);
        gmsx_csr_free(t);
        t = nullptr;
        CHECK(gmsx_csr_generate_weighted(GMSX_GEN_KRONECKER, 8, 4, GMSX_RELABEL_AUTO, 2, &t) == GMSX_OK);
        gmsx_csr_free(t);
        CHECK(gmsx_csr_save_wsg(nullptr, "x") == GMSX_ERR_INVALID && gmsx_csr_weights(nullptr) == nullptr);
    }
    gmsx_csr_free(g);
    if (failures) return 1;
    std::printf("all weighted-loader cases passed\n");
    return 0;
}
