// Stand-alone driver of reazonspeech_amd/csrc/rs_family.h for tests/test_family_host.py (built with g++, once plain and once under
// the host sanitizers).
//   dump    one line per row of the table: "<entry> <families served, a mask> <needs finalize> <hint>"
//   guard   the guard's answer for every row and every state of a context:
//           "<entry> <have context> <family> <finalized> <code> <message>"; then the same call without a message buffer must
//           give the same code (the size and frame-count queries call it that way)
//   names   "<family> <its name in the refusal texts>"
#include <stdio.h>
#include <string.h>

#include <string>

#include "../reazonspeech_amd/csrc/rs_family.h"

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "dump") {
        for (int e = 0; e < RS_ENTRY_COUNT; ++e)
            printf("%s %d %d %s\n", rs_entry_rows[e].name, rs_entry_rows[e].serves, rs_entry_rows[e].needs_final, rs_entry_rows[e].hint);
        return 0;
    }
    if (mode == "guard") {
        for (int e = 0; e < RS_ENTRY_COUNT; ++e)
            for (int have = 0; have < 2; ++have)
                for (int fam = RS_FAM_CONFORMER; fam <= RS_FAM_AVSR; ++fam)
                    for (int fin = 0; fin < 2; ++fin) {
                        char msg[512];
                        memset(msg, '#', sizeof msg);
                        msg[0] = 0;
                        const int rc = rs_family_guard((rs_entry)e, have != 0, (rs_family)fam, fin != 0, msg, sizeof msg);
                        if (memchr(msg, 0, sizeof msg) == nullptr) return 3;                     // the text is terminated inside the buffer
                        if (rs_family_guard((rs_entry)e, have != 0, (rs_family)fam, fin != 0, nullptr, 0) != rc) return 4;
                        printf("%s %d %d %d %d %s\n", rs_entry_rows[e].name, have, fam, fin, rc, msg);
                    }
        return 0;
    }
    if (mode == "names") {
        for (int fam = RS_FAM_CONFORMER; fam <= RS_FAM_AVSR; ++fam) printf("%d %s\n", fam, rs_family_name((rs_family)fam));
        return 0;
    }
    return 2;
}
