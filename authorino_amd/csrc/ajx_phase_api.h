// ajx_phase_api.h — private: the phase object of the C-ABI (include/authjx.h authjx_phase_*),
// shared by ajx_phase_api.cpp (which creates it, and links the render kernel's translation
// unit) and ajx_batcher_api.cpp (whose authjx_batcher_phase submits its requests).
#pragma once
#include "ajx_host.h"
#include "ajx_phase.h"

// One AuthConfig as the serving path sees it: borrowed objects and what the batch plan
// reads of them.
struct authjx_phase {
    int device = 0;
    const authjx_ruleset* rules = nullptr;
    const authjx_ruleset* selectors = nullptr;
    const authjx_render* prog = nullptr;
    ajx::PhaseFacts f;
};
