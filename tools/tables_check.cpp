// tables_check -- the scene compiler (mrt_tables.hip) run stand-alone on the CPU, for a sanitizer
// build (`make tables-check`: AddressSanitizer + UBSan over mrt_tables.hip, scene_builder.cpp and
// mrt_common.cpp; no GPU code, nothing preloaded).  For reference scenes 0-9, with no test hook set
// and with each of MRT_NO_BVHW, MRT_FORCE_GENERIC and MRT_NO_SIG set to 1, it builds the tables and
// prints one line "<case> <hook> <17 digest words>" (or "<case> <hook> error <mrt_last_error>");
// tools/tables_digest.py --compare checks the lines against tests/golden/tables_parent.json.
// Assets: $MRT_ASSET_DIR (unpacked: tools/pack_assets.py --unpack).
#include <cstdio>
#include <cstdlib>

#include "../miniraytracer_amd/csrc/mrt_tables.h"

int main() {
    static const char* const kHooks[] = {"MRT_NO_BVHW", "MRT_FORCE_GENERIC", "MRT_NO_SIG"};
    for (uint32_t sid = 0; sid < 10; sid++) {
        mrt_scene_blob* blob = nullptr;
        mrt_scene_view view;
        if (mrt_select_scene(sid, 1.0f, nullptr, &blob) != MRT_OK || mrt_scene_blob_view(blob, &view) != MRT_OK) {
            fprintf(stderr, "scene %u: %s\n", sid, mrt_last_error());
            return 1;
        }
        for (int setting = -1; setting < 3; setting++) {
            for (const char* h : kHooks) unsetenv(h);
            if (setting >= 0) setenv(kHooks[setting], "1", 1);
            printf("scene_%u %s", sid, setting < 0 ? "none" : kHooks[setting]);
            SceneTables T;
            if (mrt_internal_scene_tables(&view, &T) != MRT_OK) {
                printf(" error %s\n", mrt_last_error());
                continue;
            }
            uint64_t d[MRT_TABLES_DIGEST_WORDS];
            mrt_internal_tables_digest(T, d);
            for (uint64_t w : d) printf(" %016llx", (unsigned long long)w);
            printf("\n");
        }
        mrt_scene_blob_free(blob);
    }
    return 0;
}
