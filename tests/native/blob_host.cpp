// blob_host.cpp — TEST-ONLY: the reconcile-time compiler on the host, handing the compiled
// ruleset blob back to the test (tests/test_keyslot_facts.py reads the blob's tables as the
// kernels do: RulesetHdr, TrieNode, TrieChild, KeySlot of ajx_blob.h).
#include <cstdio>
#include <cstring>
#include <string>

#include "../../authorino_amd/csrc/ajx_compiler.h"

using namespace ajx;

extern "C" {

// compile `tree`; returns the blob's size (0: failed, *rc and err say why). bt_blob then
// copies the last compiled blob of this thread.
static thread_local CompiledRuleset g_last;

uint32_t bt_compile(const authjx_tree* tree, char* err, size_t cap, int* rc) {
    std::string e;
    g_last = CompiledRuleset();
    *rc = compile_tree(tree, &g_last, &e);
    if (err && cap) std::snprintf(err, cap, "%s", e.c_str());
    return *rc == AUTHJX_OK ? (uint32_t)g_last.blob.size() : 0u;
}

void bt_blob(uint8_t* out) { std::memcpy(out, g_last.blob.data(), g_last.blob.size()); }

// the offsets and sizes of the tables the test reads
void bt_layout(uint32_t* out) {
    const RulesetHdr* h = (const RulesetHdr*)g_last.blob.data();
    out[0] = h->flags & kFlagFastOk ? 1u : 0u;
    out[1] = h->n_trie_nodes;
    out[2] = h->off_trie_nodes;
    out[3] = h->off_trie_children;
    out[4] = h->off_key_slots;
    out[5] = h->key_slots_log2;
    out[6] = h->key_probes;
    out[7] = h->key_mult;
    out[8] = h->off_literals;
    out[9] = (uint32_t)sizeof(TrieNode);
    out[10] = (uint32_t)sizeof(TrieChild);
    out[11] = (uint32_t)sizeof(KeySlot);
    out[12] = h->lean_feat;
}

// the home slot of (sig, len, parent) in the last blob's key table
uint32_t bt_home(uint64_t sig, uint32_t len, uint32_t parent) {
    const RulesetHdr* h = (const RulesetHdr*)g_last.blob.data();
    return key_slot_hash(sig, len, parent, h->key_slots_log2, h->key_mult);
}

}  // extern "C"
