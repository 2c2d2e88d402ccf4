// The one way a VITLORA_* environment switch is read (INTEGRATION.md section 5 lists every switch, its default and when it is read).
#pragma once
#include <cstdlib>

// integer switch: atoi of the value when set
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
inline double env_double(const char* name, double dflt) {
    const char* e = getenv(name);
    return e ? atof(e) : dflt;
}
// on / off switch: a default-on flag is off only when the value starts with '0', a default-off flag is on only when it starts with '1'
inline bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    if (!e) return dflt;
    return dflt ? e[0] != '0' : e[0] == '1';
}
