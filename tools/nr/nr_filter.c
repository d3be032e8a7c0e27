/*
 * The filter table the noise-reduction recorders hand the reference (tools/nr/nr.mk renames
 * FilterInfo to NrFilterInfo where the reference reads it): the layout of the firmware's
 * FilterDescriptor, one entry, writable, so a case can name any filter width.  The recorders point
 * ts.filters_p at a path with id 0.
 */
#include <stdint.h>

struct { uint8_t id; const char* name; uint16_t width; } NrFilterInfo[1];

void nr_set_filter_width(uint16_t width) { NrFilterInfo[0].width = width; }
