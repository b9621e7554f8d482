// Under AGRIFLY_USE_REFERENCE_TYPES the facade must not bring its look-alikes: the same translation unit would then define
// Simulation::SimulationObject6DOF twice and not compile.  Checked the other way round: the facade's base IS the class
// declared in the agri-fly tree's header (its _radio member type and the tree-only RadioMessageDecoded(uint8_t const[])
// constructor exist).  Compiled -fsyntax-only against the tree's headers by oracle/Makefile (_ref/dropin_base.ok).
#include <type_traits>
#include "Components/Logic/QuadcopterLogic.hpp"
#include "agrifly/Quadcopter_T.hpp"
typedef agrifly::Quadcopter_T<Onboard::QuadcopterLogic> Q;
static_assert(std::is_base_of<Simulation::SimulationObject6DOF, Q>::value, "IS-A SimulationObject6DOF");
static_assert(std::is_abstract<Simulation::SimulationObject6DOF>::value, "the tree's abstract class");
static_assert(!std::is_abstract<Q>::value, "every pure virtual of the tree's class is overridden");
static_assert(std::is_constructible<RadioTypes::RadioMessageDecoded, uint8_t const *>::value, "the reference's decoder, not the look-alike");
static_assert(sizeof(RadioTypes::RadioMessageDecoded::RawMessage) == AFE_RADIO_PACKET_SIZE, "23-byte uplink");
static_assert(sizeof(TelemetryPacket::data_packet_t) == AFE_TELEMETRY_PACKET_SIZE, "30-byte telemetry packet");
int main() { return 0; }
