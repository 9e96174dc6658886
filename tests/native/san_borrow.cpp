// san_borrow.cpp — TEST-ONLY: the host build of the lean walk (ajx_lean.h) under
// AddressSanitizer / UBSan with every spare-budget policy of lean_borrow_host.cpp (tokens of
// the next sub-window taken early): members of every kind moved over every offset of a
// sub-window pair, whole, broken and cut short, at every misalignment. Besides the
// sanitizers' own reports it checks that each policy gives policy 0's tri-state, error
// index, results and capture row. Built by `make -f lean_borrow.mk san_borrow`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/authjx.h"

extern "C" {
void* ht_compile(const authjx_tree* tree, int32_t* status, char* err, size_t cap, int* rc);
void ht_free(void* h);
int ht_eval_lean_row(void* h, const uint8_t* doc, uint32_t len, uint32_t mis, uint8_t* res, int32_t* err,
                     uint64_t* row_out);
void ht_lean_spare(uint32_t policy, uint32_t k, uint64_t seed);
uint64_t ht_lean_early(void);
void ht_lean_keep(int keep);
}

static const char* kSel[] = {"k", "num", "t", "n", "o.in", "o", "sq", "long", "o.deep.in", "arr.0", "arr.2", "arr.3.in", "arr.4"};
static const char* kVal[] = {"v", "12", "true", "", "abc", "", "", "x", "abc", "w", "true", "abc", "12"};
static const char* kMembers[] = {
    "\"k\":\"v\"", "\"k\":\"0123456789abcdef\"", "\"long\":\"The quick brown fox jumps over the lazy dog, twice.\"",
    "\"num\":12", "\"num\":123456", "\"t\":true", "\"n\":null", "\"u\":-1.5e10", "\"o\":{\"in\":\"abc\"}", "\"o\":{}",
    "\"o\":{\"deep\":{\"in\":\"abc\"}}", "\"sq\":{\"x\":{\"y\":[1,{\"q\":2}]},\"w\":\"}\"}", "\"sq\":[[],[[]],{\"a\":\"]\"}]",
    "\"k\":\"a\\\\\\\"b\"", "\"arr\":[\"w\",\"x\",true,{\"in\":\"abc\"},12,null]", "\"arr\":[12,[1,2],true,{\"in\":\"abc\",\"z\":{}},12]",
    "\"arr\":[]"};
static const uint32_t kPolicies[][3] = {{1, 1, 0}, {1, 2, 0}, {1, 3, 0}, {2, 0, 0}, {3, 0, 1}, {3, 0, 2}, {3, 0, 3}};

struct Out {
    int tri;
    int32_t err;
    std::vector<uint8_t> res;
    std::vector<uint64_t> row;
    bool operator==(const Out& o) const { return tri == o.tri && (tri < 0 || (err == o.err && res == o.res && row == o.row)); }
};

static Out scan(void* h, const std::string& d, uint32_t mis, uint32_t np) {
    Out o{0, -1, std::vector<uint8_t>(np, 0), std::vector<uint64_t>(1 + np, 0)};
    o.tri = ht_eval_lean_row(h, (const uint8_t*)d.data(), (uint32_t)d.size(), mis, o.res.data(), &o.err, o.row.data());
    return o;
}

int main() {
    const uint32_t np = sizeof kSel / sizeof *kSel;
    std::vector<authjx_pattern> pats;
    std::vector<authjx_node> nodes;
    for (uint32_t i = 0; i < np; i++) {
        pats.push_back(authjx_pattern{kSel[i], (uint32_t)strlen(kSel[i]), 1 + (int)(i & 1), kVal[i], (uint32_t)strlen(kVal[i])});
        nodes.push_back(authjx_node{AUTHJX_NODE_PATTERN, -1, -1, (int)i});
    }
    int root = -1;
    for (int i = (int)np - 1; i >= 0; i--) {
        nodes.push_back(authjx_node{AUTHJX_NODE_AND, i, root, -1});
        root = (int)nodes.size() - 1;
    }
    const authjx_tree tree{pats.data(), np, nodes.data(), (uint32_t)nodes.size(), root};
    int rc = 0;
    char err[256];
    void* h = ht_compile(&tree, nullptr, err, sizeof err, &rc);
    if (!h) return printf("compile: %s\n", err), 2;
    long docs = 0, lean = 0, bad = 0;
    for (int keep = 0; keep < 2; keep++) {
        ht_lean_keep(keep);
        for (size_t m = 0; m < sizeof kMembers / sizeof *kMembers; m++)
            for (uint32_t pad = 0; pad < 71; pad++)
                for (int form = 0; form < 3; form++) {
                    std::string d = "{\"pad\":\"" + std::string(pad, 'p') + "\"," + kMembers[m] + ",\"z\":{\"a\":1}}";
                    const size_t at = 10 + pad;  // the member's first byte
                    if (form == 1) d[at + (pad * 7 + m) % (d.size() - at)] = "]}(:\"x"[(pad + m) % 6];
                    if (form == 2) d.resize(at + 1 + (pad * 5 + m) % (d.size() - at));
                    const uint32_t mis = (uint32_t)((pad * 3 + m + form) % 16);
                    ht_lean_spare(0, 0, 0);
                    const Out base = scan(h, d, mis, np);
                    docs++;
                    lean += base.tri >= 0;
                    for (const auto& p : kPolicies) {
                        ht_lean_spare(p[0], p[1], p[2]);
                        if (!(scan(h, d, mis, np) == base)) {
                            if (bad++ < 10) printf("MISMATCH policy %u/%u mis %u doc=%s\n", p[0], p[1], mis, d.c_str());
                        }
                    }
                }
    }
    ht_free(h);
    printf("docs %ld lean_decided %ld early %llu mismatches %ld\n", docs, lean, (unsigned long long)ht_lean_early(), bad);
    return bad || !ht_lean_early() ? 1 : 0;
}
